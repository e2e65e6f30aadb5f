// abi_log_values_many.inl — C ABI: icp_evaluator_log_values_many, the log values of many states under many evaluators
// (kernels_evaluate.hip; the reference's logger scores every named evaluator on every logged sample:
// JSONAcceptRejectLogger.scala:84-106, ProductEvaluators.scala:50-54).
//
// Item b's value, aux and status are the bits icp_evaluator_log_value(evaluators[b], thetas[b]) gives on a fresh evaluator: the same
// instance, the same exact searches, the one-item launchers' reductions (k_eval_reduce) and finish_eval on the host.  Items run in
// chunks (their candidate lists within kEvalCandBudget ints).  Per chunk: the instances; the model-side sample points of the items
// that share a target packed into ONE query list and searched as one surface search (and one nearest-vertex search for the
// boundary-aware items, which come first in the list) — the target streams once per chunk, not once per item; one target-to-model
// search per item against its own instance; every reduction in one launch.  Everything is enqueued on the first context's stream,
// with ONE synchronisation at the end.  The call owns all it writes: no memo, bind state, state slot, filed hint or result area of
// an evaluator or a context is read or written.  An item's bits depend neither on the other items nor on the chunks.

namespace {
constexpr size_t kEvalCandBudget = (size_t)160 << 20;  // ints of candidate lists per round of searches (640 MiB)
constexpr int kEvalMaxChunk = 256;                     // items per chunk
constexpr int kEvalHintElems = 1024;                   // elements of the strided subset a query's hint is taken from
size_t eval_cand(int K, int n_elems) { return K > 0 ? (size_t)(query_kpad(K) + 4) * cand_stride(n_elems) : 0; }

struct EvalSides {  // what enqueue_eval_searches / _reductions run for an evaluator
  bool m2t, t2m, nnv_m, nnv_t;
  int Km, Kt;
};
EvalSides eval_sides(const icp_evaluator& e) {
  const icp_evaluator_params& p = e.prm;
  const icp_ctx& c = *e.ctx;
  EvalSides s{};
  s.m2t = p.kind == ICP_EVAL_HAUSDORFF || p.mode != ICP_TARGET_TO_MODEL;
  s.t2m = p.kind == ICP_EVAL_HAUSDORFF || p.mode != ICP_MODEL_TO_TARGET;
  s.Km = s.m2t ? (p.kind == ICP_EVAL_HAUSDORFF ? c.N : p.n_model_ids) : 0;
  s.Kt = s.t2m ? e.Kt : 0;
  const bool aware = p.kind == ICP_EVAL_COLLECTIVE_AVG_HAUSDORFF_BOUNDARY_AWARE && c.target.n_boundary > 0;
  s.nnv_m = s.m2t && aware;
  s.nnv_t = s.t2m && aware;
  return s;
}
}  // namespace

extern "C" {

int icp_evaluator_log_values_many(int32_t n_items, icp_evaluator* const* evaluators, const double* const* thetas, double* values,
                                  double* aux, int32_t* status) {
  std::vector<int> item_status;
  std::vector<double> val_out, aux_out;
  int rc = guard([&] {
    require(n_items > 0 && evaluators && thetas && values && status, "null argument");
    require(n_items <= 65535, "at most 65,535 items a call");
    const int B = n_items;
    std::vector<icp_ctx*> ctxs(B);
    for (int b = 0; b < B; ++b) {
      require(evaluators[b] && thetas[b], "null argument");
      ctxs[b] = evaluators[b]->ctx;
    }
    icp_ctx& lead = *ctxs[0];
    require_one_model(B, ctxs.data(), "items of one call share a device and a model");
    const int r = lead.r, N = lead.N, T = lead.T;
    for (int b = 0; b < B; ++b) require_finite(thetas[b], 10 + (size_t)r, "theta contains a non-finite value");
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    lock_contexts(B, ctxs.data(), locks);
    Bound _b(&lead);
    hipStream_t st = lead.stream;
    // ---- the plan: chunks of items whose candidate lists fit the budget
    std::vector<EvalSides> side(B);
    std::vector<int> chunk_at{0};
    {
      size_t acc = 0;
      for (int b = 0; b < B; ++b) {
        const EvalSides& s = side[b] = eval_sides(*evaluators[b]);
        const DeviceMesh& tg = ctxs[b]->target;
        const size_t need = eval_cand(s.Km, tg.T) + (s.nnv_m ? eval_cand(s.Km, tg.V) : 0) + eval_cand(s.Kt, T) + (s.nnv_t ? eval_cand(s.Kt, N) : 0);
        const int n = b - chunk_at.back();
        if (n > 0 && (n >= kEvalMaxChunk || acc + need > kEvalCandBudget)) { chunk_at.push_back(b); acc = 0; }
        acc += need;
      }
      chunk_at.push_back(B);
    }
    const int n_chunks = (int)chunk_at.size() - 1;
    // a chunk's layout: item b's instance in slot b - chunk_at[i]; its model-side points at mq[b] of the packed lists (grouped by
    // target, the items that need nearest vertices first), its target-side results at tq[b]; its spheres in slot sph[b] (or none)
    struct Group { icp_ctx* c; size_t q0; int K, Knnv; };
    struct ChunkPlan {
      std::vector<Group> groups;
      size_t gather, n_gather, items, n_items, reduce, n_reduce;
    };
    std::vector<ChunkPlan> plan(n_chunks);
    std::vector<size_t> mq(B, 0), tq(B, 0);
    std::vector<int> sph(B, -1);
    size_t C = 1, MQ = 1, TQ = 1, SP = 1;
    for (int i = 0; i < n_chunks; ++i) {
      const int b0 = chunk_at[i], b1 = chunk_at[i + 1];
      C = std::max(C, (size_t)(b1 - b0));
      size_t m = 0, t = 0;
      int sp = 0;
      std::vector<char> placed(b1 - b0, 0);
      for (int b = b0; b < b1; ++b) {
        if (side[b].t2m) { tq[b] = t; t += side[b].Kt; sph[b] = sp++; }
        if (!side[b].m2t || placed[b - b0]) continue;
        Group g{ctxs[b], m, 0, 0};
        for (int want_nnv = 1; want_nnv >= 0; --want_nnv) {
          for (int k = b; k < b1; ++k)
            if (side[k].m2t && ctxs[k] == g.c && (int)side[k].nnv_m == want_nnv) {
              placed[k - b0] = 1;
              mq[k] = m; m += side[k].Km;
            }
          if (want_nnv) g.Knnv = (int)(m - g.q0);
        }
        g.K = (int)(m - g.q0);
        plan[i].groups.push_back(g);
      }
      MQ = std::max(MQ, m); TQ = std::max(TQ, t); SP = std::max(SP, (size_t)sp);
    }
    // ---- call-wide buffers and the chunk's slots
    DBuf<double> coeffs, res, x, Pm, cpm, d2m, cpt, d2t;
    DBuf<float4> spheres;
    DBuf<int> trim, nnvm, hintm, hintnm, trit, nnvt, hintt, hintnt;
    const size_t sf4 = sphere_floats4(T);
    {
      PackedCoeffs hc((size_t)B * r);
      for (int b = 0; b < B; ++b) hc.add(thetas[b], r);
      hc.upload(coeffs);
    }
    res.alloc((size_t)B * 8);
    x.alloc(C * 3 * N); spheres.alloc(SP * sf4);
    Pm.alloc(3 * MQ); cpm.alloc(3 * MQ); d2m.alloc(MQ); trim.alloc(MQ); nnvm.alloc(MQ); hintm.alloc(MQ); hintnm.alloc(MQ);
    cpt.alloc(3 * TQ); d2t.alloc(TQ); trit.alloc(TQ); nnvt.alloc(TQ); hintt.alloc(TQ); hintnt.alloc(TQ);
    // ---- records: instances, sphere items, gathers, reductions (searches below: they need the scratch's size first)
    InstancePlan inst;
    std::vector<size_t> inst_at(n_chunks + 1, 0);
    std::vector<MetItem> h_item;
    std::vector<EvalGather> h_gather;
    std::vector<EvalReduce> h_reduce;
    for (int i = 0; i < n_chunks; ++i) {
      ChunkPlan& cp = plan[i];
      const int b0 = chunk_at[i], b1 = chunk_at[i + 1];
      inst.boundary();
      cp.gather = h_gather.size(); cp.items = h_item.size(); cp.reduce = h_reduce.size();
      for (int b = b0; b < b1; ++b) {
        const EvalSides& s = side[b];
        const icp_evaluator_params& p = evaluators[b]->prm;
        const DeviceMesh& tg = ctxs[b]->target;
        double* xb = x.p + (size_t)(b - b0) * 3 * N;
        double* o = res.p + (size_t)b * 8;
        inst.add(lead, coeffs.p + (size_t)b * r, ctxs[b]->pose_of(thetas[b]), xb);
        if (s.t2m) h_item.push_back(MetItem{xb, spheres.p + (size_t)sph[b] * sf4, nullptr});
        if (s.m2t && s.Km > 0) h_gather.push_back(EvalGather{xb, Pm.p + 3 * mq[b], s.Km});
        // (enqueue_eval_searches / _reductions: which reduction, over which list, into which of the eight results)
        for (int half = 0; half < 2; ++half) {
          if (!(half == 0 ? s.m2t : s.t2m)) continue;
          const int K = half == 0 ? s.Km : s.Kt;
          const double* d2 = half == 0 ? d2m.p + mq[b] : d2t.p + tq[b];
          const int* nnv = half == 0 ? nnvm.p + mq[b] : nnvt.p + tq[b];
          const bool flags = half == 0 ? s.nnv_m : s.nnv_t;
          if (p.kind == ICP_EVAL_INDEPENDENT_POINT_DISTANCE)
            h_reduce.push_back(EvalReduce{kEvalGauss, K, d2, p.gauss_mean, p.gauss_sigma, nullptr, nullptr, 0, o + 4 * half});
          else if (p.kind == ICP_EVAL_HAUSDORFF)
            h_reduce.push_back(EvalReduce{kEvalMax, K, d2, 0.0, 1.0, nullptr, nullptr, 0, o + 4 * half + 1});
          else  // (target side: the nearest MODEL vertex against the TARGET's flags, sic — SURVEY App. D5)
            h_reduce.push_back(EvalReduce{kEvalStats, K, d2, 0.0, 1.0, flags ? tg.boundary.p : nullptr, flags ? nnv : nullptr, tg.V, o + 4 * half});
        }
      }
      inst_at[i + 1] = inst.groups.size();
      cp.n_gather = h_gather.size() - cp.gather; cp.n_items = h_item.size() - cp.items; cp.n_reduce = h_reduce.size() - cp.reduce;
    }
    // ---- searches: four rounds per chunk — the packed model-side lists against their targets' surfaces (0) and vertices (2), every
    // item's target-side points against its instance's surface (1) and vertices (3).  Pass 0 sizes the scratch, pass 1 makes the records.
    struct Round { size_t first, n; int kpad, filter, kmax; };
    std::vector<MetSearch> h_search;
    std::vector<Round> rounds((size_t)n_chunks * 4);
    size_t cand_max = 1, q_max = 1;
    DBuf<double> thr2;
    DBuf<float4> qrec;
    DBuf<float> thrA;
    DBuf<int> cnt, cand;
    for (int pass = 0; pass < 2; ++pass) {
      h_search.clear();
      if (pass == 1) { thr2.alloc(q_max); qrec.alloc(q_max); thrA.alloc(q_max); cnt.alloc(q_max); cand.alloc(cand_max); }
      size_t co = 0, qo = 0;  // the round's scratch cursors
      Round* rd = nullptr;
      auto begin_round = [&](Round& r_) { rd = &r_; r_ = Round{h_search.size(), 0, 0, 0, 0}; co = 0; qo = 0; };
      auto end_round = [&] { rd->n = h_search.size() - rd->first; cand_max = std::max(cand_max, co); q_max = std::max(q_max, qo); };
      auto qbuf = [&](int K, int n_elems) {
        const size_t kp = (size_t)query_kpad(K) + 4, cap = eval_cand(K, n_elems);
        QueryBuffers qb{nullptr, nullptr, nullptr, nullptr, nullptr, cap};
        if (pass == 1) qb = QueryBuffers{thr2.p + qo, qrec.p + qo, thrA.p + qo, cnt.p + qo, cand.p + co, cap};
        qo += kp; co += cap;
        return qb;
      };
      auto add_surface = [&](int Te, const double* verts, const int* tris, const float4* sph_, int K, const double* Pq, int* hint,
                             double* cp_, double* d2, int* tri) {
        QueryBuffers qb = qbuf(K, Te);
        qb.thr2 = nullptr;
        MetSearch m{};
        m.kind = 0;
        m.s = make_surface_task(Te, verts, tris, sph_, K, Pq, hint, qb, cp_, d2, tri);
        m.fblocks = Te > 0 ? filter_grid_blocks(m.s.tblocks, m.s.ksplit) : 0;
        m.hint_step = std::max(1, Te / kEvalHintElems);
        rd->kpad = std::max(rd->kpad, m.s.Kpad); rd->filter = std::max(rd->filter, m.fblocks); rd->kmax = std::max(rd->kmax, K);
        h_search.push_back(m);
      };
      // (hint: the first corner of the triangle the surface point lies on)
      auto add_vertex = [&](int Ve, const double* verts, int K, const double* Pq, int* hint, int* idx, const int* htri, const int* htris) {
        QueryBuffers qb = qbuf(K, Ve);
        qb.qrec = nullptr; qb.thrA = nullptr;
        MetSearch m{};
        m.kind = 1;
        m.v = make_vertex_task(Ve, verts, K, Pq, hint, qb, nullptr, idx);
        m.fblocks = filter_grid_blocks(m.v.vblocks, m.v.ksplit);
        m.hint_step = 0;
        m.hint_tri = htri; m.hint_tris = htris;
        rd->kpad = std::max(rd->kpad, m.v.Kpad); rd->filter = std::max(rd->filter, m.fblocks); rd->kmax = std::max(rd->kmax, K);
        h_search.push_back(m);
      };
      for (int i = 0; i < n_chunks; ++i) {
        const ChunkPlan& cp = plan[i];
        const int b0 = chunk_at[i], b1 = chunk_at[i + 1];
        search_chains_hint(b1 - b0);
        begin_round(rounds[4 * (size_t)i + 0]);
        for (const Group& g : cp.groups) {
          const DeviceMesh& tg = g.c->target;
          if (g.K > 0)
            add_surface(tg.T, tg.verts.p, tg.tris.p, tg.spheres.p, g.K, Pm.p + 3 * g.q0, hintm.p + g.q0, cpm.p + 3 * g.q0, d2m.p + g.q0, trim.p + g.q0);
        }
        end_round();
        begin_round(rounds[4 * (size_t)i + 1]);
        for (int b = b0; b < b1; ++b)
          if (side[b].t2m && side[b].Kt > 0)
            add_surface(T, x.p + (size_t)(b - b0) * 3 * N, lead.tris.p, spheres.p + (size_t)sph[b] * sf4, side[b].Kt, evaluators[b]->d_tpts,
                        hintt.p + tq[b], cpt.p + 3 * tq[b], d2t.p + tq[b], trit.p + tq[b]);
        end_round();
        begin_round(rounds[4 * (size_t)i + 2]);
        for (const Group& g : cp.groups) {
          const DeviceMesh& tg = g.c->target;
          if (g.Knnv > 0) add_vertex(tg.V, tg.verts.p, g.Knnv, cpm.p + 3 * g.q0, hintnm.p + g.q0, nnvm.p + g.q0, trim.p + g.q0, tg.tris.p);
        }
        end_round();
        begin_round(rounds[4 * (size_t)i + 3]);
        for (int b = b0; b < b1; ++b)
          if (side[b].nnv_t && side[b].Kt > 0)
            add_vertex(N, x.p + (size_t)(b - b0) * 3 * N, side[b].Kt, cpt.p + 3 * tq[b], hintnt.p + tq[b], nnvt.p + tq[b], trit.p + tq[b],
                       lead.tris.p);
        end_round();
      }
      search_chains_hint(1);
    }
    DBuf<InstanceItem> d_inst;
    DBuf<InstanceGroup> d_grp;
    DBuf<MetItem> d_item;
    DBuf<EvalGather> d_gather;
    DBuf<EvalReduce> d_reduce;
    DBuf<MetSearch> d_search;
    {
      NullStreamBatch _nb;
      inst.upload(d_inst, d_grp);
      d_item.upload(h_item.data(), h_item.size());
      d_gather.upload(h_gather.data(), h_gather.size());
      d_reduce.upload(h_reduce.data(), h_reduce.size());
      d_search.upload(h_search.data(), h_search.size());
    }
    // ---- launches
    HIP_OK(hipMemsetAsync(res.p, 0, sizeof(double) * 8 * (size_t)B, st));  // (as enqueue_eval_searches: a side that does not run leaves zeros)
    for (int i = 0; i < n_chunks; ++i) {
      const ChunkPlan& cp = plan[i];
      launch_instance_many(st, (int)(inst_at[i + 1] - inst_at[i]), N, d_grp.p + inst_at[i], d_inst.p);  // ModelFittingParameters.scala:108-110
      launch_met_items(st, (int)cp.n_items, N, T, lead.tris.p, lead.tri_order.p, lead.adj_off.p, lead.adj.p, false, d_item.p + cp.items);
      int kmax = 0;
      for (size_t g = cp.gather; g < cp.gather + cp.n_gather; ++g) kmax = std::max(kmax, h_gather[g].K);
      launch_eval_gather(st, (int)cp.n_gather, kmax, d_gather.p + cp.gather);
      for (int k = 0; k < 4; ++k) {
        const Round& rd = rounds[4 * (size_t)i + k];
        launch_met_searches(st, (int)rd.n, rd.kpad, rd.filter, rd.kmax, d_search.p + rd.first);
      }
      launch_eval_reduce(st, (int)cp.n_reduce, d_reduce.p + cp.reduce);
    }
    std::vector<double> hr((size_t)B * 8);
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpy(hr.data(), res.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost));
    item_status.assign(B, ICP_OK);
    val_out.assign(B, 0.0);
    aux_out.assign((size_t)B * 4, 0.0);
    for (int b = 0; b < B; ++b)
      item_status[b] = finish_eval(evaluators[b], &hr[(size_t)b * 8], &val_out[b], &aux_out[(size_t)b * 4]);
  });
  if (rc != ICP_OK) return rc;
  std::memcpy(values, val_out.data(), sizeof(double) * val_out.size());
  if (aux) std::memcpy(aux, aux_out.data(), sizeof(double) * aux_out.size());
  // (the rule of icp_chain_step_batched_collect: an empty boundary-aware set is that item's answer, not the call's failure)
  report_item_status(n_items, item_status, status, [](int code) { return icp_status_string(code); });
  for (int b = 0; b < n_items; ++b)
    if (item_status[b] != ICP_OK && item_status[b] != ICP_ERR_EMPTY) {
      g_err = icp_status_string(item_status[b]);
      return item_status[b];
    }
  return ICP_OK;
}

}  // extern "C"
