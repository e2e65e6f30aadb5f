// abi_metrics_many.inl — C ABI: icp_mesh_metrics_many, the registration metrics and Dice of many meshes (kernels_metrics.hip).
//
// Item b's out[0..4] are the bits icp_mesh_metrics(ctxs[b], thetas[b]) gives: the same instance, the same exact searches (model
// vertices -> target surface, their surface points -> nearest target vertex where the target has a boundary, target vertices -> the
// instance's surface) and k_dist_stats' reductions at the same block size.  out[5..8] = Dice and its three counts.  Items run in
// chunks (their candidate lists within kMetCandBudget ints), every launch of a chunk carries all its items; everything is enqueued on
// the first context's stream, with ONE synchronisation at the end.  An item's bits depend neither on the other items nor on the chunks.

namespace {
constexpr size_t kMetCandBudget = (size_t)160 << 20;  // ints of candidate lists per round of searches (640 MiB)
constexpr int kMetMaxChunk = 64;                      // items per chunk
constexpr int kMetDiceRange = 32768;                  // Dice samples per search
constexpr int kMetHintElems = 1024;                   // elements of the strided subset a query's hint is taken from
size_t met_cand(int K, int n_elems) { return (size_t)(query_kpad(K) + 4) * cand_stride(n_elems); }

// the target's vertex-to-triangle adjacency (as the model's, vertex_adjacency), its vertex normals and box: made for Dice on the
// first call that needs them (enqueued on `st`; valid once that call has synchronised)
void ensure_target_geometry(icp_ctx& c, hipStream_t st, std::vector<MetBoxJob>& boxes) {
  const int V = c.target.V, T = c.target.T;
  std::vector<int32_t> tris((size_t)3 * T);
  if (T > 0) HIP_OK(hipMemcpy(tris.data(), c.target.tris.p, sizeof(int32_t) * tris.size(), hipMemcpyDeviceToHost));
  std::vector<int> off, adj;
  vertex_adjacency(V, T, tris.data(), off, adj);
  {
    NullStreamBatch _nb;
    c.tgt_adj_off.upload(off.data(), off.size());
    c.tgt_adj.upload(adj.data(), adj.size());
  }
  c.tgt_normals.alloc((size_t)3 * V);
  c.tgt_box.alloc(6);
  launch_vertex_normals(st, V, c.target.verts.p, c.target.tris.p, c.tgt_adj_off.p, c.tgt_adj.p, c.tgt_normals.p);
  boxes.push_back(MetBoxJob{c.target.verts.p, V, nullptr, c.tgt_box.p, nullptr});
}
}  // namespace

extern "C" {

int icp_mesh_metrics_many(int32_t n_items, icp_ctx* const* ctxs, const double* const* thetas, int32_t dice_samples, uint64_t dice_seed,
                          double* out, int32_t* status) {
  std::vector<int> item_status;
  std::vector<double> res_out;
  int rc = guard([&] {
    require(n_items > 0 && ctxs && thetas && out && status, "null argument");
    require(n_items <= 65535, "at most 65,535 items a call");
    require(dice_samples >= 0 && dice_samples <= (1 << 24), "dice_samples must lie in [0, 2^24]");
    const int B = n_items;
    for (int b = 0; b < B; ++b) require(ctxs[b] && thetas[b], "null argument");
    icp_ctx& lead = *ctxs[0];
    require_one_model(B, ctxs, "items of one call share a device and a model");
    const int r = lead.r, N = lead.N, T = lead.T;
    for (int b = 0; b < B; ++b) require_finite(thetas[b], 10 + (size_t)r, "theta contains a non-finite value");
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    const std::vector<icp_ctx*> distinct = lock_contexts(B, ctxs, locks);
    Bound _b(&lead);
    hipStream_t st = lead.stream;
    const int S = dice_samples;
    const bool dice = S > 0;
    // ---- the plan: chunks of items whose candidate lists fit the budget
    int Mmax = 1;
    std::vector<size_t> need(B);
    for (int b = 0; b < B; ++b) {
      const DeviceMesh& tg = ctxs[b]->target;
      Mmax = std::max(Mmax, tg.V);
      need[b] = met_cand(N, tg.T) + met_cand(tg.V, T) + (tg.n_boundary > 0 ? met_cand(N, tg.V) : 0);
    }
    std::vector<int> chunk_at{0};
    {
      size_t acc = 0;
      for (int b = 0; b < B; ++b) {
        const int n = b - chunk_at.back();
        if (n > 0 && (n >= kMetMaxChunk || acc + need[b] > kMetCandBudget)) { chunk_at.push_back(b); acc = 0; }
        acc += need[b];
      }
      chunk_at.push_back(B);
    }
    const int n_chunks = (int)chunk_at.size() - 1;
    int C = 1;
    for (int i = 0; i < n_chunks; ++i) C = std::max(C, chunk_at[i + 1] - chunk_at[i]);
    // ---- call-wide buffers and the chunk's per-item slots
    DBuf<double> coeffs, res, boxes, x, normals, d2m, cpm, d2t;
    DBuf<float4> spheres;
    DBuf<int> nonfinite, trim, nnv, hintm, hintn, hintt;
    DBuf<unsigned> counts;
    const size_t sf4 = sphere_floats4(T);
    {
      PackedCoeffs hc((size_t)B * r);
      for (int b = 0; b < B; ++b) hc.add(thetas[b], r);
      hc.upload(coeffs);
    }
    res.alloc((size_t)B * 12); boxes.alloc((size_t)B * 6); nonfinite.alloc(B); counts.alloc((size_t)B * 3);
    x.alloc((size_t)C * 3 * N); spheres.alloc((size_t)C * sf4);
    if (dice) normals.alloc((size_t)C * 3 * N);
    d2m.alloc((size_t)C * N); cpm.alloc((size_t)C * 3 * N); trim.alloc((size_t)C * N); nnv.alloc((size_t)C * N);
    hintm.alloc((size_t)C * N); hintn.alloc((size_t)C * N);
    d2t.alloc((size_t)C * Mmax); hintt.alloc((size_t)C * Mmax);
    // ---- the targets' Dice geometry (once per context)
    std::vector<MetBoxJob> tboxes;
    std::vector<icp_ctx*> made;
    if (dice)
      for (icp_ctx* c : distinct)
        if (!c->tgt_geo_valid) { ensure_target_geometry(*c, st, tboxes); made.push_back(c); }
    // ---- records: instances, items, boxes, searches, stats, Dice ranges (slot j of a chunk = item chunk_at[i] + j)
    InstancePlan inst;  // a chunk's instances: whole groups, inst_at[i] .. inst_at[i + 1] - 1
    std::vector<size_t> inst_at(n_chunks + 1, 0);
    std::vector<MetItem> h_item(B);
    std::vector<MetBoxJob> h_box(B);
    for (int i = 0; i < n_chunks; ++i) {
      inst.boundary();
      for (int b = chunk_at[i]; b < chunk_at[i + 1]; ++b) {
        const size_t j = (size_t)(b - chunk_at[i]);
        double* xb = x.p + j * 3 * N;
        inst.add(lead, coeffs.p + (size_t)b * r, ctxs[b]->pose_of(thetas[b]), xb);
        h_item[b] = MetItem{xb, spheres.p + j * sf4, dice ? normals.p + j * 3 * N : nullptr};
        h_box[b] = MetBoxJob{xb, N, dice ? ctxs[b]->tgt_box.p : nullptr, boxes.p + (size_t)b * 6, nonfinite.p + b};
      }
      inst_at[i + 1] = inst.groups.size();
    }
    struct Round { size_t first, n; int kpad, filter, kmax; size_t cand, qslots; };
    std::vector<MetSearch> h_search;
    std::vector<MetStats> h_stats;
    std::vector<MetDice> h_dice;
    struct ChunkPlan { Round r1, r2; size_t stats_big, n_big, stats_small, n_small; std::vector<Round> dice; std::vector<std::pair<size_t, size_t>> dice_rec; };
    std::vector<ChunkPlan> plan(n_chunks);
    size_t cand_max = 1, q_max = 1, dice_pts_max = 1;
    DBuf<double> thr2, dP;
    DBuf<float4> qrec;
    DBuf<float> thrA;
    DBuf<int> cnt, cand, dA, dB, dhA, dhB;
    // pass 0 sizes the scratch, pass 1 makes the records with its pointers
    for (int pass = 0; pass < 2; ++pass) {
      h_search.clear(); h_stats.clear(); h_dice.clear();
      if (pass == 1) {
        thr2.alloc(q_max); qrec.alloc(q_max); thrA.alloc(q_max); cnt.alloc(q_max); cand.alloc(cand_max);
        if (dice) { dP.alloc(3 * dice_pts_max); dA.alloc(dice_pts_max); dB.alloc(dice_pts_max); dhA.alloc(dice_pts_max); dhB.alloc(dice_pts_max); }
      }
      size_t co = 0, qo = 0;  // the round's scratch cursors
      auto begin_round = [&](Round& rd) { rd = Round{h_search.size(), 0, 0, 0, 0, 0, 0}; co = 0; qo = 0; };
      auto end_round = [&](Round& rd) {
        rd.n = h_search.size() - rd.first; rd.cand = co; rd.qslots = qo;
        cand_max = std::max(cand_max, co); q_max = std::max(q_max, qo);
      };
      auto qbuf = [&](int K, int n_elems, QueryBuffers& qb) {
        const size_t kp = (size_t)query_kpad(K) + 4, cap = met_cand(K, n_elems);
        if (pass == 1) qb = QueryBuffers{thr2.p + qo, qrec.p + qo, thrA.p + qo, cnt.p + qo, cand.p + co, cap};
        else qb = QueryBuffers{nullptr, nullptr, nullptr, nullptr, nullptr, cap};
        qo += kp; co += cap;
      };
      auto add_surface = [&](Round& rd, int Te, const double* verts, const int* tris, const float4* sph, int K, const double* Pq, int* hint,
                             double* cp, double* d2, int* tri) {
        QueryBuffers qb;
        qbuf(K, Te, qb);
        qb.thr2 = nullptr;
        MetSearch m{};
        m.kind = 0;
        m.s = make_surface_task(Te, verts, tris, sph, K, Pq, hint, qb, cp, d2, tri);
        m.fblocks = Te > 0 ? filter_grid_blocks(m.s.tblocks, m.s.ksplit) : 0;
        m.hint_step = std::max(1, Te / kMetHintElems);
        rd.kpad = std::max(rd.kpad, m.s.Kpad); rd.filter = std::max(rd.filter, m.fblocks); rd.kmax = std::max(rd.kmax, K);
        h_search.push_back(m);
      };
      auto add_vertex = [&](Round& rd, int Ve, const double* verts, int K, const double* Pq, int* hint, int* idx, const int* htri,
                            const int* htris) {
        QueryBuffers qb;
        qbuf(K, Ve, qb);
        qb.qrec = nullptr; qb.thrA = nullptr;
        MetSearch m{};
        m.kind = 1;
        m.v = make_vertex_task(Ve, verts, K, Pq, hint, qb, nullptr, idx);
        m.fblocks = filter_grid_blocks(m.v.vblocks, m.v.ksplit);
        m.hint_step = htri ? 0 : std::max(1, Ve / kMetHintElems);
        m.hint_tri = htri; m.hint_tris = htris;
        rd.kpad = std::max(rd.kpad, m.v.Kpad); rd.filter = std::max(rd.filter, m.fblocks); rd.kmax = std::max(rd.kmax, K);
        h_search.push_back(m);
      };
      for (int i = 0; i < n_chunks; ++i) {
        ChunkPlan& cp = plan[i];
        const int b0 = chunk_at[i], b1 = chunk_at[i + 1];
        search_chains_hint(2 * (b1 - b0));
        begin_round(cp.r1);
        for (int b = b0; b < b1; ++b) {
          const size_t j = (size_t)(b - b0);
          const DeviceMesh& tg = ctxs[b]->target;
          // reconstruction -> target: every model vertex against the target surface
          add_surface(cp.r1, tg.T, tg.verts.p, tg.tris.p, tg.spheres.p, N, x.p + j * 3 * N, hintm.p + j * N, cpm.p + j * 3 * N,
                      d2m.p + j * N, trim.p + j * N);
          // target -> reconstruction: every target vertex against the instance's surface
          add_surface(cp.r1, T, x.p + j * 3 * N, lead.tris.p, spheres.p + j * sf4, tg.V, tg.verts.p, hintt.p + j * Mmax, nullptr,
                      d2t.p + j * Mmax, nullptr);
        }
        end_round(cp.r1);
        search_chains_hint(b1 - b0);
        begin_round(cp.r2);
        for (int b = b0; b < b1; ++b) {  // the surface points' nearest target vertices, where the target has a boundary
          const size_t j = (size_t)(b - b0);
          const DeviceMesh& tg = ctxs[b]->target;
          if (tg.n_boundary > 0)
            add_vertex(cp.r2, tg.V, tg.verts.p, N, cpm.p + j * 3 * N, hintn.p + j * N, nnv.p + j * N, trim.p + j * N, tg.tris.p);
        }
        end_round(cp.r2);
        // the three distance lists of every item, grouped by the one-item path's block size
        for (int big = 1; big >= 0; --big) {
          (big ? cp.stats_big : cp.stats_small) = h_stats.size();
          for (int b = b0; b < b1; ++b) {
            const size_t j = (size_t)(b - b0);
            const DeviceMesh& tg = ctxs[b]->target;
            const bool flags = tg.n_boundary > 0;
            double* o = res.p + (size_t)b * 12;
            if ((N > 4096) == (big == 1)) {
              h_stats.push_back(MetStats{N, d2m.p + j * N, nullptr, nullptr, 0, o + 0});
              h_stats.push_back(MetStats{N, d2m.p + j * N, flags ? tg.boundary.p : nullptr, flags ? nnv.p + j * N : nullptr, tg.V, o + 4});
            }
            if ((tg.V > 4096) == (big == 1)) h_stats.push_back(MetStats{tg.V, d2t.p + j * Mmax, nullptr, nullptr, 0, o + 8});
          }
          (big ? cp.n_big : cp.n_small) = h_stats.size() - (big ? cp.stats_big : cp.stats_small);
        }
        // Dice: ranges of at most kMetDiceRange samples, in groups whose candidate lists fit the budget
        cp.dice.clear(); cp.dice_rec.clear();
        if (dice) {
          std::vector<std::pair<int, int>> ranges;  // (item, first sample)
          for (int b = b0; b < b1; ++b)
            for (int s0 = 0; s0 < S; s0 += kMetDiceRange) ranges.emplace_back(b, s0);
          size_t k = 0;
          while (k < ranges.size()) {
            size_t acc = 0, pts = 0, k1 = k;
            for (; k1 < ranges.size(); ++k1) {
              const int n = std::min(kMetDiceRange, S - ranges[k1].second);
              const size_t nd = met_cand(n, N) + met_cand(n, ctxs[ranges[k1].first]->target.V);
              if (k1 > k && (acc + nd > kMetCandBudget || k1 - k >= 2 * (size_t)kMetMaxChunk)) break;
              acc += nd; pts += n;
            }
            dice_pts_max = std::max(dice_pts_max, pts);
            search_chains_hint((int)(2 * (k1 - k)));
            cp.dice.emplace_back();
            Round& rd = cp.dice.back();
            begin_round(rd);
            const size_t rec0 = h_dice.size();
            size_t po = 0;
            for (size_t q = k; q < k1; ++q) {
              const int b = ranges[q].first, s0 = ranges[q].second, n = std::min(kMetDiceRange, S - s0);
              const size_t j = (size_t)(b - b0);
              icp_ctx& c = *ctxs[b];
              double* Pq = pass == 1 ? dP.p + 3 * po : nullptr;
              int* iA = pass == 1 ? dA.p + po : nullptr;
              int* iB = pass == 1 ? dB.p + po : nullptr;
              add_vertex(rd, N, x.p + j * 3 * N, n, Pq, pass == 1 ? dhA.p + po : nullptr, iA, nullptr, nullptr);
              add_vertex(rd, c.target.V, c.target.verts.p, n, Pq, pass == 1 ? dhB.p + po : nullptr, iB, nullptr, nullptr);
              h_dice.push_back(MetDice{n, s0, boxes.p + (size_t)b * 6, Pq, iA, iB, x.p + j * 3 * N, pass == 1 ? normals.p + j * 3 * N : nullptr,
                                       N, c.target.verts.p, c.tgt_normals.p, c.target.V, counts.p + (size_t)b * 3});
              po += n;
            }
            end_round(rd);
            cp.dice_rec.emplace_back(rec0, h_dice.size() - rec0);
            k = k1;
          }
        }
      }
      search_chains_hint(1);
    }
    // (the target geometry above is complete before any record reads it: same stream; its pointers exist since ensure_target_geometry)
    DBuf<InstanceItem> d_inst;
    DBuf<InstanceGroup> d_grp;
    DBuf<MetItem> d_item;
    DBuf<MetBoxJob> d_box, d_tbox;
    DBuf<MetSearch> d_search;
    DBuf<MetStats> d_stats;
    DBuf<MetDice> d_dice;
    {
      NullStreamBatch _nb;
      inst.upload(d_inst, d_grp);
      d_item.upload(h_item.data(), h_item.size());
      d_box.upload(h_box.data(), h_box.size());
      if (!tboxes.empty()) d_tbox.upload(tboxes.data(), tboxes.size());
      d_search.upload(h_search.data(), h_search.size());
      d_stats.upload(h_stats.data(), h_stats.size());
      if (!h_dice.empty()) d_dice.upload(h_dice.data(), h_dice.size());
    }
    // ---- launches
    HIP_OK(hipMemsetAsync(counts.p, 0, sizeof(unsigned) * 3 * (size_t)B, st));
    launch_met_box(st, (int)tboxes.size(), d_tbox.p);
    auto run = [&](const Round& rd) { launch_met_searches(st, (int)rd.n, rd.kpad, rd.filter, rd.kmax, d_search.p + rd.first); };
    for (int i = 0; i < n_chunks; ++i) {
      const ChunkPlan& cp = plan[i];
      const int b0 = chunk_at[i], nb = chunk_at[i + 1] - b0;
      launch_instance_many(st, (int)(inst_at[i + 1] - inst_at[i]), N, d_grp.p + inst_at[i], d_inst.p);  // ModelFittingParameters.scala:108-110
      launch_met_items(st, nb, N, T, lead.tris.p, lead.tri_order.p, lead.adj_off.p, lead.adj.p, dice, d_item.p + b0);
      launch_met_box(st, nb, d_box.p + b0);
      run(cp.r1);
      run(cp.r2);
      launch_met_stats(st, (int)cp.n_big, true, d_stats.p + cp.stats_big);
      launch_met_stats(st, (int)cp.n_small, false, d_stats.p + cp.stats_small);
      for (size_t g = 0; g < cp.dice.size(); ++g) {
        const auto& dr = cp.dice_rec[g];
        int nmax = 1;
        for (size_t q = dr.first; q < dr.first + dr.second; ++q) nmax = std::max(nmax, h_dice[q].n);
        launch_met_samples(st, (int)dr.second, nmax, dice_seed, d_dice.p + dr.first);
        run(cp.dice[g]);
        launch_met_dice_count(st, (int)dr.second, nmax, d_dice.p + dr.first);
      }
    }
    std::vector<double> hr((size_t)B * 12);
    std::vector<unsigned> hk((size_t)B * 3);
    std::vector<int> hn(B);
    HIP_OK(hipStreamSynchronize(st));
    for (icp_ctx* c : made) c->tgt_geo_valid = true;
    HIP_OK(hipMemcpy(hr.data(), res.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hk.data(), counts.p, sizeof(unsigned) * hk.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hn.data(), nonfinite.p, sizeof(int) * B, hipMemcpyDeviceToHost));
    item_status.assign(B, ICP_OK);
    res_out.assign((size_t)B * 9, NAN);
    for (int b = 0; b < B; ++b) {
      if (hn[b] != 0) { item_status[b] = ICP_ERR_NOT_FINITE; continue; }
      const double* h = &hr[(size_t)b * 12];
      double* o = &res_out[(size_t)b * 9];
      o[0] = h[0] / h[2];  // (as icp_mesh_metrics)
      o[1] = std::max(h[1], h[9]);
      o[2] = h[6] > 0.0 ? h[4] / h[6] : NAN;
      o[3] = h[6] > 0.0 ? h[5] : NAN;
      o[4] = h[6];
      if (dice) {
        const double na = hk[3 * (size_t)b], nb = hk[3 * (size_t)b + 1], nab = hk[3 * (size_t)b + 2];
        o[5] = na + nb > 0.0 ? 2.0 * nab / (na + nb) : NAN;
        o[6] = na; o[7] = nb; o[8] = nab;
      }
    }
  });
  if (rc != ICP_OK) return rc;
  std::memcpy(out, res_out.data(), sizeof(double) * res_out.size());
  return report_item_status(n_items, item_status, status, [](int) { return "an item's mesh is not finite"; });
}

}  // extern "C"
