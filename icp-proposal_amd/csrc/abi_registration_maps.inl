// abi_registration_maps.inl — C ABI: icp_registration_maps_many and icp_distance_summaries_many, the per-vertex result of many
// registrations and the maps a chain's samples imply (kernels_maps.hip behind the metrics' searches, kernels_metrics.hip).
//
// An item is a state on a context.  Its instance, its triangle spheres, its non-finite count and its searches — model vertices ->
// target surface, the surface points' nearest target vertices where the target has a boundary, target vertices -> the instance's
// surface — are icp_mesh_metrics_many's launches on icp_mesh_metrics_many's records, so every row is the exact lexicographic
// (d², index) minimum the one-item entry points give.  A direction nobody asked for is not searched.  Items run in chunks (their
// candidate lists within kMetCandBudget ints, their rows within kMapChunkDoubles doubles of staging); every launch of a chunk carries
// all its items, the chunk's rows go back to the caller behind it, and the next chunk takes the same buffers: device memory does not
// grow with the number of items.  Everything is enqueued on the first context's stream, with ONE synchronisation at the end.  An
// item's bits depend neither on the other items, nor on their order, nor on the chunks.

namespace {
constexpr size_t kMapChunkDoubles = (size_t)4 << 20;  // staging rows of a chunk: 32 MiB (an item always fits)
constexpr int kMapMaxChunk = 64;                      // items per chunk

// copies of a chunk's rows to the caller's arrays, any element type: neighbours on both sides go as ONE copy (HostCopies, in bytes)
struct RowCopies {
  struct Run { const char* dev; char* host; size_t n; };
  std::vector<Run> runs;
  void add(const void* dev, void* host, size_t bytes) {
    const char* d = (const char*)dev;
    char* h = (char*)host;
    if (!runs.empty() && runs.back().dev + runs.back().n == d && runs.back().host + runs.back().n == h) runs.back().n += bytes;
    else runs.push_back(Run{d, h, bytes});
  }
  void issue(hipStream_t st) {
    for (const Run& c : runs) HIP_OK(hipMemcpyAsync(c.host, c.dev, c.n, hipMemcpyDeviceToHost, st));
    runs.clear();
  }
};

// the searches of a list of items, chunk by chunk: plan() lays the call out and makes the records, run(i) enqueues chunk i up to its
// last search.  Slot j of a chunk = item chunk_at[i] + j; an item's target -> instance rows start t_off[b] target vertices into the
// chunk's arrays (the items' vertex counts differ).
struct MapSearches {
  int B = 0, N = 0, T = 0, r = 0;
  icp_ctx* const* ctxs = nullptr;
  const double* const* thetas = nullptr;
  MapWant w{};
  std::vector<int> chunk_at;
  std::vector<size_t> t_off;
  int C = 1;
  size_t t_rows = 1;  // target vertices of the largest chunk
  DBuf<double> coeffs, boxes, x, d2m, cpm, d2t, cpt, thr2;
  DBuf<float4> spheres, qrec;
  DBuf<float> thrA;
  DBuf<int> nonfinite, trim, nnv, hintm, hintn, hintt, trit, cnt, cand;
  DBuf<InstanceItem> d_inst;
  DBuf<InstanceGroup> d_grp;
  DBuf<MetItem> d_item;
  DBuf<MetBoxJob> d_box;
  DBuf<MetSearch> d_search;
  struct Round { size_t first = 0, n = 0; int kpad = 0, filter = 0, kmax = 0; };
  std::vector<Round> r1, r2;
  std::vector<size_t> inst_at;

  int n_chunks() const { return (int)chunk_at.size() - 1; }
  int slot(int b, int i) const { return b - chunk_at[i]; }
  bool flags_of(int b) const { return w.boundary && ctxs[b]->target.n_boundary > 0; }

  void plan(icp_ctx& lead) {
    N = lead.N; T = lead.T; r = lead.r;
    const size_t cap = test_chunk_doubles("ICP_TEST_MAPS_CHUNK_DOUBLES", kMapChunkDoubles);
    // ---- chunks: candidate lists of the wanted searches within the budget, rows within the staging
    chunk_at.assign(1, 0);
    t_off.assign(B, 0);
    {
      size_t acc = 0, rows = 0, tv = 0;
      for (int b = 0; b < B; ++b) {
        const DeviceMesh& tg = ctxs[b]->target;
        const size_t need = (w.m2t ? met_cand(N, tg.T) : 0) + (w.t2m ? met_cand(tg.V, T) : 0) + (flags_of(b) ? met_cand(N, tg.V) : 0);
        const size_t doubles = (w.m2t ? 6 * (size_t)N : 0) + (w.t2m ? 6 * (size_t)tg.V : 0);
        const int n = b - chunk_at.back();
        if (n > 0 && (n >= kMapMaxChunk || acc + need > kMetCandBudget || rows + doubles > cap)) {
          chunk_at.push_back(b);
          acc = 0; rows = 0; tv = 0;
        }
        t_off[b] = tv;
        acc += need; rows += doubles; tv += (size_t)tg.V;
        t_rows = std::max(t_rows, tv);
      }
      chunk_at.push_back(B);
    }
    for (int i = 0; i < n_chunks(); ++i) C = std::max(C, chunk_at[i + 1] - chunk_at[i]);
    // ---- buffers of a chunk
    const size_t sf4 = sphere_floats4(T);
    {
      PackedCoeffs hc((size_t)B * r);
      for (int b = 0; b < B; ++b) hc.add(thetas[b], r);
      hc.upload(coeffs);
    }
    nonfinite.alloc(B); boxes.alloc((size_t)C * 6); x.alloc((size_t)C * 3 * N);
    if (w.m2t) {
      d2m.alloc((size_t)C * N); hintm.alloc((size_t)C * N);
      if (w.m2t_cp || w.boundary) cpm.alloc((size_t)C * 3 * N);
      if (w.m2t_tri || w.boundary) trim.alloc((size_t)C * N);
      if (w.boundary) { nnv.alloc((size_t)C * N); hintn.alloc((size_t)C * N); }
    }
    if (w.t2m) {
      spheres.alloc((size_t)C * sf4);
      d2t.alloc(t_rows); hintt.alloc(t_rows);
      if (w.t2m_cp) cpt.alloc(3 * t_rows);
      if (w.t2m_tri) trit.alloc(t_rows);
    }
    // ---- the rounds' scratch: per query slots and candidate lists of the largest round
    size_t q_max = 1, cand_max = 1;
    for (int i = 0; i < n_chunks(); ++i) {
      size_t q1 = 0, c1 = 0, q2 = 0, c2 = 0;
      for (int b = chunk_at[i]; b < chunk_at[i + 1]; ++b) {
        const DeviceMesh& tg = ctxs[b]->target;
        if (w.m2t) { q1 += (size_t)query_kpad(N) + 4; c1 += met_cand(N, tg.T); }
        if (w.t2m) { q1 += (size_t)query_kpad(tg.V) + 4; c1 += met_cand(tg.V, T); }
        if (flags_of(b)) { q2 += (size_t)query_kpad(N) + 4; c2 += met_cand(N, tg.V); }
      }
      q_max = std::max({q_max, q1, q2}); cand_max = std::max({cand_max, c1, c2});
    }
    thr2.alloc(q_max); qrec.alloc(q_max); thrA.alloc(q_max); cnt.alloc(q_max); cand.alloc(cand_max);
    // ---- records: instances, items, boxes, searches
    InstancePlan inst;
    std::vector<MetItem> h_item(B);
    std::vector<MetBoxJob> h_box(B);
    std::vector<MetSearch> h_search;
    inst_at.assign(n_chunks() + 1, 0);
    r1.assign(n_chunks(), Round{}); r2.assign(n_chunks(), Round{});
    size_t qo = 0, co = 0;
    auto qbuf = [&](int K, int n_elems) {
      const size_t kp = (size_t)query_kpad(K) + 4, cp = met_cand(K, n_elems);
      QueryBuffers qb{thr2.p + qo, qrec.p + qo, thrA.p + qo, cnt.p + qo, cand.p + co, cp};
      qo += kp; co += cp;
      return qb;
    };
    auto grow = [](Round& rd, int kpad, int fblocks, int K) {
      rd.kpad = std::max(rd.kpad, kpad); rd.filter = std::max(rd.filter, fblocks); rd.kmax = std::max(rd.kmax, K);
    };
    auto add_surface = [&](Round& rd, int Te, const double* verts, const int* tris, const float4* sph, int K, const double* Pq, int* hint,
                           double* cp, double* d2, int* tri) {
      QueryBuffers qb = qbuf(K, Te);
      qb.thr2 = nullptr;
      MetSearch m{};
      m.kind = 0;
      m.s = make_surface_task(Te, verts, tris, sph, K, Pq, hint, qb, cp, d2, tri);
      m.fblocks = Te > 0 ? filter_grid_blocks(m.s.tblocks, m.s.ksplit) : 0;
      m.hint_step = std::max(1, Te / kMetHintElems);
      grow(rd, m.s.Kpad, m.fblocks, K);
      h_search.push_back(m);
    };
    for (int i = 0; i < n_chunks(); ++i) {
      const int b0 = chunk_at[i], b1 = chunk_at[i + 1];
      inst.boundary();
      for (int b = b0; b < b1; ++b) {
        const size_t j = (size_t)(b - b0);
        double* xb = x.p + j * 3 * N;
        inst.add(lead, coeffs.p + (size_t)b * r, ctxs[b]->pose_of(thetas[b]), xb);
        h_item[b] = MetItem{xb, w.t2m ? spheres.p + j * sf4 : nullptr, nullptr};
        h_box[b] = MetBoxJob{xb, N, nullptr, boxes.p + j * 6, nonfinite.p + b};
      }
      inst_at[i + 1] = inst.groups.size();
      search_chains_hint((int)((w.m2t ? 1 : 0) + (w.t2m ? 1 : 0)) * (b1 - b0));
      r1[i].first = h_search.size(); qo = 0; co = 0;
      for (int b = b0; b < b1; ++b) {
        const size_t j = (size_t)(b - b0);
        const DeviceMesh& tg = ctxs[b]->target;
        if (w.m2t)  // every model vertex against the target surface
          add_surface(r1[i], tg.T, tg.verts.p, tg.tris.p, tg.spheres.p, N, x.p + j * 3 * N, hintm.p + j * N,
                      cpm.p ? cpm.p + j * 3 * N : nullptr, d2m.p + j * N, trim.p ? trim.p + j * N : nullptr);
        if (w.t2m)  // every target vertex against the instance's surface
          add_surface(r1[i], T, x.p + j * 3 * N, lead.tris.p, spheres.p + j * sf4, tg.V, tg.verts.p, hintt.p + t_off[b],
                      cpt.p ? cpt.p + 3 * t_off[b] : nullptr, d2t.p + t_off[b], trit.p ? trit.p + t_off[b] : nullptr);
      }
      r1[i].n = h_search.size() - r1[i].first;
      search_chains_hint(b1 - b0);
      r2[i].first = h_search.size(); qo = 0; co = 0;
      for (int b = b0; b < b1; ++b) {  // the surface points' nearest target vertices, where the target has a boundary
        if (!flags_of(b)) continue;
        const size_t j = (size_t)(b - b0);
        const DeviceMesh& tg = ctxs[b]->target;
        QueryBuffers qb = qbuf(N, tg.V);
        qb.qrec = nullptr; qb.thrA = nullptr;
        MetSearch m{};
        m.kind = 1;
        m.v = make_vertex_task(tg.V, tg.verts.p, N, cpm.p + j * 3 * N, hintn.p + j * N, qb, nullptr, nnv.p + j * N);
        m.fblocks = filter_grid_blocks(m.v.vblocks, m.v.ksplit);
        m.hint_step = 0;  // a corner of the triangle the point lies on
        m.hint_tri = trim.p + j * N; m.hint_tris = tg.tris.p;
        grow(r2[i], m.v.Kpad, m.fblocks, N);
        h_search.push_back(m);
      }
      r2[i].n = h_search.size() - r2[i].first;
    }
    search_chains_hint(1);
    {
      NullStreamBatch _nb;
      inst.upload(d_inst, d_grp);
      d_item.upload(h_item.data(), h_item.size());
      d_box.upload(h_box.data(), h_box.size());
      d_search.upload(h_search.data(), h_search.size());
    }
  }

  void run(hipStream_t st, icp_ctx& lead, int i) {
    const int b0 = chunk_at[i], nb = chunk_at[i + 1] - b0;
    launch_instance_many(st, (int)(inst_at[i + 1] - inst_at[i]), N, d_grp.p + inst_at[i], d_inst.p);  // ModelFittingParameters.scala:108-110
    if (w.t2m) launch_met_items(st, nb, N, T, lead.tris.p, lead.tri_order.p, lead.adj_off.p, lead.adj.p, false, d_item.p + b0);
    launch_met_box(st, nb, d_box.p + b0);
    launch_met_searches(st, (int)r1[i].n, r1[i].kpad, r1[i].filter, r1[i].kmax, d_search.p + r1[i].first);
    launch_met_searches(st, (int)r2[i].n, r2[i].kpad, r2[i].filter, r2[i].kmax, d_search.p + r2[i].first);
  }
};

// the checks every call of this file makes before anything runs; returns the lead context
icp_ctx& maps_check_items(int B, icp_ctx* const* ctxs, const double* const* thetas) {
  for (int b = 0; b < B; ++b) require(ctxs[b] && thetas[b], "null argument");
  require_one_model(B, ctxs, "items of one call share a device and a model");
  for (int b = 0; b < B; ++b) require_finite(thetas[b], 10 + (size_t)ctxs[0]->r, "theta contains a non-finite value");
  return *ctxs[0];
}
}  // namespace

extern "C" {

int icp_registration_maps_many(int32_t n_items, icp_ctx* const* ctxs, const double* const* thetas, double* const* m2t_point,
                               int32_t* const* m2t_triangle, double* const* m2t_distance, uint8_t* const* m2t_on_boundary,
                               double* const* t2m_point, int32_t* const* t2m_triangle, double* const* t2m_distance, int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(ctxs && thetas && status, "null argument");
    require(m2t_point || m2t_triangle || m2t_distance || m2t_on_boundary || t2m_point || t2m_triangle || t2m_distance,
            "at least one output must be asked for");
    const int B = n_items;
    for (int b = 0; b < B; ++b)
      require((!m2t_point || m2t_point[b]) && (!m2t_triangle || m2t_triangle[b]) && (!m2t_distance || m2t_distance[b]) &&
                  (!m2t_on_boundary || m2t_on_boundary[b]) && (!t2m_point || t2m_point[b]) && (!t2m_triangle || t2m_triangle[b]) &&
                  (!t2m_distance || t2m_distance[b]),
              "null argument");
    icp_ctx& lead = maps_check_items(B, ctxs, thetas);
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    lock_contexts(B, ctxs, locks);
    Bound _b(&lead);
    hipStream_t st = lead.stream;
    MapSearches ms;
    ms.B = B; ms.ctxs = ctxs; ms.thetas = thetas;
    ms.w.m2t = m2t_point || m2t_triangle || m2t_distance || m2t_on_boundary;
    ms.w.t2m = t2m_point || t2m_triangle || t2m_distance;
    ms.w.m2t_cp = m2t_point != nullptr; ms.w.m2t_tri = m2t_triangle != nullptr;
    ms.w.boundary = false;
    if (m2t_on_boundary)
      for (int b = 0; b < B; ++b) ms.w.boundary = ms.w.boundary || ctxs[b]->target.n_boundary > 0;
    ms.w.t2m_cp = t2m_point != nullptr; ms.w.t2m_tri = t2m_triangle != nullptr;
    ms.plan(lead);
    const int N = ms.N, C = ms.C;
    // ---- the epilogue's rows and records
    DBuf<double> distm, distt;
    DBuf<unsigned char> flag;
    if (m2t_distance) distm.alloc((size_t)C * N);
    if (m2t_on_boundary) flag.alloc((size_t)C * N);
    if (t2m_distance) distt.alloc(ms.t_rows);
    std::vector<MapItem> h_map(B);
    std::vector<int> kmax(ms.n_chunks(), 0);
    for (int i = 0; i < ms.n_chunks(); ++i)
      for (int b = ms.chunk_at[i]; b < ms.chunk_at[i + 1]; ++b) {
        const size_t j = (size_t)ms.slot(b, i), to = ms.t_off[b];
        const DeviceMesh& tg = ctxs[b]->target;
        MapItem& it = h_map[b];
        it = MapItem{};
        it.nonfinite = ms.nonfinite.p + b;
        if (ms.w.m2t) {
          it.m2t = MapSide{N, ms.d2m.p + j * N, ms.cpm.p ? ms.cpm.p + j * 3 * N : nullptr, ms.trim.p ? ms.trim.p + j * N : nullptr,
                           distm.p ? distm.p + j * N : nullptr};
          kmax[i] = std::max(kmax[i], N);
        }
        if (ms.w.t2m) {
          it.t2m = MapSide{tg.V, ms.d2t.p + to, ms.cpt.p ? ms.cpt.p + 3 * to : nullptr, ms.trit.p ? ms.trit.p + to : nullptr,
                           distt.p ? distt.p + to : nullptr};
          kmax[i] = std::max(kmax[i], tg.V);
        }
        if (m2t_on_boundary) {
          it.flag = flag.p + j * N;
          if (ms.flags_of(b)) { it.nnv = ms.nnv.p + j * N; it.boundary = tg.boundary.p; it.n_flags = tg.V; }
        }
      }
    DBuf<MapItem> d_map;
    d_map.upload(h_map.data(), h_map.size());
    // ---- launches: a chunk's searches, its epilogue, its rows back to the caller
    RowCopies back;
    for (int i = 0; i < ms.n_chunks(); ++i) {
      const int b0 = ms.chunk_at[i], b1 = ms.chunk_at[i + 1];
      ms.run(st, lead, i);
      launch_map_rows(st, b1 - b0, kmax[i], d_map.p + b0);
      auto rows = [&](auto* const* out, size_t per_vertex, auto pick) {  // one output of every item of the chunk: (rows, vertices)
        if (!out) return;
        for (int b = b0; b < b1; ++b) {
          const std::pair<const void*, int> src = pick(h_map[b]);
          back.add(src.first, out[b], sizeof(**out) * per_vertex * (size_t)src.second);
        }
        back.issue(st);
      };
      using Src = std::pair<const void*, int>;
      rows(m2t_point, 3, [](const MapItem& it) { return Src(it.m2t.cp, it.m2t.K); });
      rows(m2t_triangle, 1, [](const MapItem& it) { return Src(it.m2t.tri, it.m2t.K); });
      rows(m2t_distance, 1, [](const MapItem& it) { return Src(it.m2t.dist, it.m2t.K); });
      rows(m2t_on_boundary, 1, [](const MapItem& it) { return Src(it.flag, it.m2t.K); });
      rows(t2m_point, 3, [](const MapItem& it) { return Src(it.t2m.cp, it.t2m.K); });
      rows(t2m_triangle, 1, [](const MapItem& it) { return Src(it.t2m.tri, it.t2m.K); });
      rows(t2m_distance, 1, [](const MapItem& it) { return Src(it.t2m.dist, it.t2m.K); });
    }
    std::vector<int> hn(B);
    HIP_OK(hipMemcpyAsync(hn.data(), ms.nonfinite.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    item_status.assign(B, ICP_OK);
    for (int b = 0; b < B; ++b)
      if (hn[b] != 0) item_status[b] = ICP_ERR_NOT_FINITE;
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int) { return "an item's mesh is not finite"; });
}

int icp_distance_summaries_many(int32_t n_sets, icp_ctx* const* ctxs, const int32_t* n_samples, const double* const* theta_sets,
                                double* const* m2t_mean, double* const* m2t_max, double* const* t2m_mean, double* const* t2m_max,
                                int32_t* status) {
  std::vector<int> set_status;
  int rc = guard([&] {
    require(n_sets >= 1 && n_sets <= 65535, "n_sets must lie in [1, 65535]");
    require(ctxs && n_samples && theta_sets && status, "null argument");
    require(m2t_mean || m2t_max || t2m_mean || t2m_max, "at least one output must be asked for");
    const int n = n_sets;
    size_t total = 0;
    for (int m = 0; m < n; ++m) {
      require(ctxs[m] && theta_sets[m] && (!m2t_mean || m2t_mean[m]) && (!m2t_max || m2t_max[m]) && (!t2m_mean || t2m_mean[m]) &&
                  (!t2m_max || t2m_max[m]),
              "null argument");
      require(n_samples[m] >= 1, "a set holds at least one sample");
      total += (size_t)n_samples[m];
    }
    require(total <= ((size_t)1 << 24), "at most 2^24 samples a call");
    // ---- the sets' samples as one list of items
    const size_t P = 10 + (size_t)ctxs[0]->r;
    std::vector<icp_ctx*> ictx;
    std::vector<const double*> ith;
    std::vector<int> set_at(n + 1, 0);
    ictx.reserve(total); ith.reserve(total);
    for (int m = 0; m < n; ++m) {
      for (int s = 0; s < n_samples[m]; ++s) { ictx.push_back(ctxs[m]); ith.push_back(theta_sets[m] + (size_t)s * P); }
      set_at[m + 1] = (int)ictx.size();
    }
    const int B = (int)total;
    icp_ctx& lead = maps_check_items(B, ictx.data(), ith.data());
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    lock_contexts(n, ctxs, locks);
    Bound _b(&lead);
    hipStream_t st = lead.stream;
    MapSearches ms;
    ms.B = B; ms.ctxs = ictx.data(); ms.thetas = ith.data();
    ms.w.m2t = m2t_mean || m2t_max;
    ms.w.t2m = t2m_mean || t2m_max;
    ms.plan(lead);
    const int N = ms.N, C = ms.C;
    int Mmax = 1;
    for (int m = 0; m < n; ++m) Mmax = std::max(Mmax, ctxs[m]->target.V);
    // ---- the maps' rows (at the slot of a set's last sample), what an open set carries between chunks (two of each: a chunk may
    // close one set and open the next), the sets' non-finite words
    DBuf<double> meanm, maxm, meant, maxt, accm, acct;
    DBuf<int> bad;
    if (m2t_mean) meanm.alloc((size_t)C * N);
    if (m2t_max) maxm.alloc((size_t)C * N);
    if (t2m_mean) meant.alloc(ms.t_rows);
    if (t2m_max) maxt.alloc(ms.t_rows);
    if (ms.w.m2t) accm.alloc((size_t)4 * N);
    if (ms.w.t2m) acct.alloc((size_t)4 * Mmax);
    bad.alloc(n);
    std::vector<MapSumSeg> h_seg;
    struct Done { int set; size_t j, to; };  // a set that ends in the chunk: where its rows are
    std::vector<size_t> seg_at(ms.n_chunks() + 1, 0);
    std::vector<std::vector<Done>> done(ms.n_chunks());
    std::vector<int> kmax(ms.n_chunks(), 0);
    {
      int m = 0;
      for (int i = 0; i < ms.n_chunks(); ++i) {
        const int b0 = ms.chunk_at[i], b1 = ms.chunk_at[i + 1];
        int b = b0;
        while (b < b1) {
          while (set_at[m + 1] <= b) ++m;
          const int e = std::min(b1, set_at[m + 1]), M = ctxs[m]->target.V;
          const int first = b == set_at[m], last = e == set_at[m + 1];
          const size_t j = (size_t)(b - b0), jl = (size_t)(e - 1 - b0), to = ms.t_off[b], tl = ms.t_off[e - 1];
          if (ms.w.m2t) {
            h_seg.push_back(MapSumSeg{N, e - b, n_samples[m], first, last, ms.d2m.p + j * N, ms.nonfinite.p + b,
                                      accm.p + (size_t)((i + 1) & 1) * 2 * N, accm.p + (size_t)(i & 1) * 2 * N, bad.p + m,
                                      meanm.p ? meanm.p + jl * N : nullptr, maxm.p ? maxm.p + jl * N : nullptr});
            kmax[i] = std::max(kmax[i], N);
          }
          if (ms.w.t2m) {
            h_seg.push_back(MapSumSeg{M, e - b, n_samples[m], first, last, ms.d2t.p + to, ms.nonfinite.p + b,
                                      acct.p + (size_t)((i + 1) & 1) * 2 * Mmax, acct.p + (size_t)(i & 1) * 2 * Mmax, bad.p + m,
                                      meant.p ? meant.p + tl : nullptr, maxt.p ? maxt.p + tl : nullptr});
            kmax[i] = std::max(kmax[i], M);
          }
          if (last) done[i].push_back(Done{m, jl, tl});
          b = e;
        }
        seg_at[i + 1] = h_seg.size();
      }
    }
    DBuf<MapSumSeg> d_seg;
    d_seg.upload(h_seg.data(), h_seg.size());
    // ---- launches: a chunk's searches, its samples folded into their sets, the finished sets' rows back to the caller
    HIP_OK(hipMemsetAsync(bad.p, 0, sizeof(int) * (size_t)n, st));
    HostCopies back;
    for (int i = 0; i < ms.n_chunks(); ++i) {
      ms.run(st, lead, i);
      launch_map_summaries(st, (int)(seg_at[i + 1] - seg_at[i]), kmax[i], d_seg.p + seg_at[i]);
      auto rows = [&](double* const* out, const DBuf<double>& src, bool target_side) {
        if (!out) return;
        for (const Done& d : done[i])
          back.add(src.p + (target_side ? d.to : d.j * N), out[d.set], target_side ? (size_t)ctxs[d.set]->target.V : (size_t)N);
        back.issue(st, false);
      };
      rows(m2t_mean, meanm, false); rows(m2t_max, maxm, false);
      rows(t2m_mean, meant, true); rows(t2m_max, maxt, true);
    }
    std::vector<int> hb(n);
    HIP_OK(hipMemcpyAsync(hb.data(), bad.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    set_status.assign(n, ICP_OK);
    for (int m = 0; m < n; ++m)
      if (hb[m] != 0) set_status[m] = ICP_ERR_NOT_FINITE;
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_sets, set_status, status, [](int) { return "a sample's mesh is not finite"; });
}

}  // extern "C"
