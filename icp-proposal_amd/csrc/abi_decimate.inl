// abi_decimate.inl — C ABI: icp_decimate_many, the decimation of many meshes to vertex subsets (kernels_decimate.hip; the step
// NonRigidIcpProposal.scala:45-46, the evaluators' constructors and apps/bfm/CreateGPModel.scala:43 start with).
//
// Item b: kk = min(k, M) farthest-point samples from `start` (equal distances go to the lowest id), the sample nearest every vertex
// along mesh edges (synchronous sweeps until no key of the item changes), and the dual triangles of those cells without duplicates.
// Every limit is checked for every item before the device is touched.  The items go through ONE buffer in rounds of at most
// kDecRoundWords 8-byte words (an item above that has a round of its own), in three regions: the inputs (ONE upload), the work arrays,
// the outputs (ONE copy back).  Per round: the selection's launches, then — only if an item of the round asks for counts, labels or
// triangles — the sweeps in groups of kDecSweepGroup with one read of the flags per group, the candidates with one read of the
// outputs, and — only if an item asks for counts or triangles — the duplicate tables, sized from the candidate counts, in a second
// buffer with one copy back.  It takes no context: the live items, the device and the stream are abi_pool_many.inl's, the rounds and
// every item's place in their regions RegionRounds' (icp_round_plan.hpp).  An item's bits depend neither on the other items, nor on
// their order, nor on the rounds, nor on the selection's route.

namespace {
constexpr size_t kDecRoundWords = (size_t)ICP_DECIMATE_ROUND_BYTES / sizeof(double);
constexpr int kDecMaxVertices = 1 << 24;
constexpr int kDecMaxTriangles = 1 << 26;
constexpr double kDecMaxMagnitude = 0x1p60;
static_assert(kDecMaxSamples == ICP_DECIMATE_MAX_POINTS, "header and kernels agree on the samples per item");

// where an item's arrays lie, in 8-byte words from the start of its part of the round's region: inputs, work arrays, outputs
struct DecLayout {
  size_t words[3];                                           // the regions' lengths: kPoolIn, kPoolWork, kPoolOut
  size_t pts, tris;                                          // inputs
  size_t D, pmax, pidx, key0, key1, tkey, keep, tpre, tblk;  // work arrays
  size_t counts, ids, spts, cover2, labels;                  // outputs
  DecLayout(size_t M, size_t T, size_t kk) {
    const size_t nblk = (M + kDecBlock - 1) / kDecBlock, tiles = (T + kScanTile - 1) / kScanTile;
    RegionCursor c;
    pts = c.take(24 * M); tris = c.take(12 * T);
    words[kPoolIn] = c.close();
    D = c.take(8 * M); pmax = c.take(16 * nblk); pidx = c.take(8 * nblk); key0 = c.take(8 * M); key1 = c.take(8 * M);
    tkey = c.take(8 * T); keep = c.take(T); tpre = c.take(4 * T); tblk = c.take(4 * tiles);
    words[kPoolWork] = c.close();
    counts = c.take(16); ids = c.take(4 * kk); spts = c.take(24 * kk); cover2 = c.take(8 * kk); labels = c.take(4 * M);
    words[kPoolOut] = c.close();
  }
};

// the duplicate table of an item with `cand` candidate triangles: a power of two of at least twice as many slots
size_t dec_table_size(size_t cand) {
  size_t s = 16;
  while (s < 2 * cand) s <<= 1;
  return s;
}
}  // namespace

extern "C" {

int icp_decimate_many(int32_t n_items, int device, const int32_t* n_points, const double* const* points, const int32_t* n_triangles,
                      const int32_t* const* cells, const int32_t* n_samples, const int32_t* starts, int32_t* counts_out,
                      int32_t* const* ids_out, double* const* points_out, double* const* cover2_out, int32_t* const* labels_out,
                      int32_t* const* cells_out, int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(n_points && points && n_triangles && n_samples && status, "null argument");
    require(counts_out || ids_out || points_out || cover2_out || labels_out || cells_out, "null argument: at least one output");
    const int B = n_items;
    // ---- validation, item by item, before the device is touched
    const std::vector<int> live = live_items(B, item_status, [&](int b) {
      const long long M = n_points[b], T = n_triangles[b], k = n_samples[b], s = starts ? starts[b] : 0;
      if (M < 1 || M > kDecMaxVertices || T < 0 || T > kDecMaxTriangles || k < 1 || k > kDecMaxSamples || s < 0 || s >= M) return false;
      if (!points[b] || (T > 0 && !(cells && cells[b]))) return false;
      return all_within(points[b], 3 * (size_t)M, kDecMaxMagnitude) && (T == 0 || ids_in_range(cells[b], 3 * (size_t)T, M));
    });
    const int n_live = (int)live.size();
    if (n_live == 0) return;

    PoolCall call(device);
    hipStream_t st = call.st;

    // test-hooks build: the size up to which the one-workgroup selection is taken (0: never), the sweeps between two reads of the flags
    int group_vertices = kDecGroupVertices, sweep_group = kDecSweepGroup;
    if (const char* v = dev_env("ICP_TEST_DECIMATE_GROUP_VERTICES")) group_vertices = std::min(std::max(std::atoi(v), 0), kDecGroupVertices);
    if (const char* v = dev_env("ICP_TEST_DECIMATE_SWEEP_GROUP")) sweep_group = std::min(std::max(std::atoi(v), 1), kDecSweepGroup);

    // ---- the plan: every item's layout; rounds = ranges of consecutive live items whose footprints fit the budget
    std::vector<DecLayout> lay;
    lay.reserve(n_live);
    RegionRounds<3> plan(test_chunk_doubles("ICP_TEST_DECIMATE_CHUNK_DOUBLES", kDecRoundWords), n_live);
    using Round = RegionRounds<3>::Round;
    for (int b : live) {
      lay.emplace_back((size_t)n_points[b], (size_t)n_triangles[b], (size_t)std::min(n_samples[b], n_points[b]));
      plan.add(lay.back().words);
    }
    const int round_items = plan.round_items;
    DBuf<double> chunk, tables;
    DBuf<DecItem> d_items;
    DBuf<DecTable> d_tables;
    DBuf<int> d_flags;
    std::vector<DecItem> h_items(n_live);
    chunk.alloc(plan.buffer_words);
    d_flags.alloc((size_t)round_items * kDecSweepGroup);
    for (const Round& rd : plan.rounds) {
      for (int q = rd.q0; q < rd.q1; ++q) {
        const int b = live[q];
        const DecLayout& l = lay[q];
        DecItem& it = h_items[q];
        it = DecItem{};
        it.M = n_points[b]; it.T = n_triangles[b]; it.kk = std::min(n_samples[b], n_points[b]); it.start = starts ? starts[b] : 0;
        it.nblk = (it.M + kDecBlock - 1) / kDecBlock;
        it.group = it.M <= group_vertices ? 1 : 0;
        const auto& at = plan.at[q];  // the item's parts, from the start of its round's regions
        double* ib = chunk.p + rd.base(kPoolIn) + at[kPoolIn];
        double* wb = chunk.p + rd.base(kPoolWork) + at[kPoolWork];
        double* ob = chunk.p + rd.base(kPoolOut) + at[kPoolOut];
        it.pts = ib + l.pts; it.tris = (const int*)(ib + l.tris);
        it.D = wb + l.D; it.pmax = wb + l.pmax; it.pidx = (int*)(wb + l.pidx);
        it.key[0] = (unsigned long long*)(wb + l.key0); it.key[1] = (unsigned long long*)(wb + l.key1);
        it.tkey = (unsigned long long*)(wb + l.tkey); it.keep = (unsigned char*)(wb + l.keep);
        it.tpre = (int*)(wb + l.tpre); it.tblk = (int*)(wb + l.tblk);
        it.counts = (int*)(ob + l.counts); it.ids = (int*)(ob + l.ids); it.spts = ob + l.spts; it.cover2 = ob + l.cover2;
        it.labels = (int*)(ob + l.labels);
        it.flags = d_flags.p + (size_t)(q - rd.q0) * kDecSweepGroup;
      }
    }
    {
      NullStreamBatch _nb;
      d_items.upload(h_items.data(), h_items.size());
    }
    std::vector<double> stage_in(plan.stage_words[kPoolIn]), stage_out(plan.stage_words[kPoolOut]), stage_tri;
    std::vector<int> h_flags((size_t)round_items * kDecSweepGroup);
    std::vector<DecTable> h_tables;

    // ---- the rounds
    for (const Round& rd : plan.rounds) {
      const int n = rd.q1 - rd.q0;
      const DecItem* items = d_items.p + rd.q0;
      double* out_dev = chunk.p + rd.base(kPoolOut);
      int m_max = 0, t_max = 0, kk_max = 0, nblk_general = 0, kk_general = 0;
      bool any_group = false, want_graph = counts_out != nullptr, want_triangles = counts_out != nullptr;
      for (int q = rd.q0; q < rd.q1; ++q) {
        const int b = live[q];
        const DecItem& it = h_items[q];
        const DecLayout& l = lay[q];
        m_max = std::max(m_max, it.M); t_max = std::max(t_max, it.T); kk_max = std::max(kk_max, it.kk);
        if (it.group) any_group = true;
        else { nblk_general = std::max(nblk_general, it.nblk); kk_general = std::max(kk_general, it.kk); }
        if (cells_out && cells_out[b]) want_graph = want_triangles = true;
        if (labels_out && labels_out[b]) want_graph = true;
        double* blk = stage_in.data() + plan.at[q][kPoolIn];
        std::memcpy(blk + l.pts, points[b], sizeof(double) * 3 * (size_t)it.M);
        if (it.T > 0) std::memcpy(blk + l.tris, cells[b], sizeof(int) * 3 * (size_t)it.T);
      }
      HIP_OK(hipMemcpyAsync(chunk.p, stage_in.data(), sizeof(double) * rd.words[kPoolIn], hipMemcpyHostToDevice, st));
      launch_dec_select(st, n, nblk_general, kk_general, any_group, items);
      std::vector<int> sweeps(n, 0);
      if (want_graph) {
        launch_dec_seed(st, n, m_max, kk_max, items);
        // the sweeps, in groups: a sweep past an item's fixpoint changes nothing, so the round runs until its slowest item is done
        int launched = 0;
        for (bool more = t_max > 0; more;) {
          if (launched > m_max + kDecSweepGroup) fail(ICP_ERR_DEVICE, "the label sweeps did not reach a fixpoint");
          HIP_OK(hipMemsetAsync(d_flags.p, 0, sizeof(int) * (size_t)n * kDecSweepGroup, st));
          for (int g = 0; g < sweep_group; ++g) launch_dec_sweep(st, n, t_max, g, (launched + g) & 1, items);
          HIP_OK(hipMemcpyAsync(h_flags.data(), d_flags.p, sizeof(int) * (size_t)n * kDecSweepGroup, hipMemcpyDeviceToHost, st));
          HIP_OK(hipStreamSynchronize(st));
          launched += sweep_group;
          more = false;
          for (int i = 0; i < n; ++i) {
            for (int g = 0; g < sweep_group; ++g) sweeps[i] += h_flags[(size_t)i * kDecSweepGroup + g] != 0;
            more = more || h_flags[(size_t)i * kDecSweepGroup + sweep_group - 1] != 0;
          }
        }
        launch_dec_candidates(st, n, std::max(m_max, t_max), launched & 1, items);
      }
      HIP_OK(hipMemcpyAsync(stage_out.data(), out_dev, sizeof(double) * rd.words[kPoolOut], hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      // k_eff and the candidate counts are here: the rows the caller gets, and the tables' sizes
      std::vector<int> k_eff(n), cand(n);
      for (int q = rd.q0; q < rd.q1; ++q) {
        int cnt[4];
        std::memcpy(cnt, stage_out.data() + plan.at[q][kPoolOut] + lay[q].counts, sizeof(cnt));
        const DecItem& it = h_items[q];
        if (cnt[0] < 1 || cnt[0] > it.kk || cnt[3] < 0 || cnt[3] > it.T) fail(ICP_ERR_DEVICE, "the decimation's counts are out of range");
        k_eff[q - rd.q0] = cnt[0]; cand[q - rd.q0] = cnt[3];
      }
      std::vector<size_t> tri_at(n);
      size_t table_words = 0, tri_words = 0;
      if (want_triangles) {
        h_tables.assign(n, DecTable{});
        for (int i = 0; i < n; ++i) table_words += region_words(12 * dec_table_size((size_t)cand[i]));
        for (int i = 0; i < n; ++i) { tri_at[i] = tri_words; tri_words += 1 + region_words(12 * (size_t)cand[i]); }
        tables.alloc(table_words + tri_words);
        size_t at = 0;
        for (int i = 0; i < n; ++i) {
          const size_t size = dec_table_size((size_t)cand[i]);
          DecTable& tb = h_tables[i];
          tb.slots = (unsigned long long*)(tables.p + at);
          tb.lowest = (unsigned*)(tables.p + at + size);
          tb.mask = (unsigned)(size - 1);
          tb.t_out = (int*)(tables.p + table_words + tri_at[i]);
          tb.cells = (int*)(tables.p + table_words + tri_at[i] + 1);
          tb.cap = cand[i];
          at += region_words(12 * size);
        }
        {
          NullStreamBatch _nb;
          d_tables.upload(h_tables.data(), h_tables.size());
        }
        HIP_OK(hipMemsetAsync(tables.p, 0xff, sizeof(double) * table_words, st));
        launch_dec_triangles(st, n, t_max, items, d_tables.p);
        stage_tri.resize(tri_words);
        HIP_OK(hipMemcpyAsync(stage_tri.data(), tables.p + table_words, sizeof(double) * tri_words, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
      }
      for (int q = rd.q0; q < rd.q1; ++q) {
        const int b = live[q], i = q - rd.q0;
        const DecLayout& l = lay[q];
        const DecItem& it = h_items[q];
        const double* blk = stage_out.data() + plan.at[q][kPoolOut];
        const size_t ke = (size_t)k_eff[i];
        if (ids_out && ids_out[b]) std::memcpy(ids_out[b], blk + l.ids, sizeof(int) * ke);
        if (points_out && points_out[b]) std::memcpy(points_out[b], blk + l.spts, sizeof(double) * 3 * ke);
        if (cover2_out && cover2_out[b]) std::memcpy(cover2_out[b], blk + l.cover2, sizeof(double) * ke);
        if (labels_out && labels_out[b]) std::memcpy(labels_out[b], blk + l.labels, sizeof(int) * (size_t)it.M);
        if (!want_triangles) continue;
        int t_out;
        std::memcpy(&t_out, stage_tri.data() + tri_at[i], sizeof(int));
        if (t_out < 0 || t_out > cand[i]) fail(ICP_ERR_DEVICE, "the decimation's triangle count is out of range");
        if (counts_out) { counts_out[3 * b] = k_eff[i]; counts_out[3 * b + 1] = t_out; counts_out[3 * b + 2] = sweeps[i]; }
        if (cells_out && cells_out[b]) std::memcpy(cells_out[b], stage_tri.data() + tri_at[i] + 1, sizeof(int) * 3 * (size_t)t_out);
      }
    }
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int) {
    return "an item is outside the limits: 1 <= n_points <= 2^24, 0 <= n_triangles <= 2^26 with ids in [0, n_points), "
           "1 <= n_samples <= 65535, 0 <= start < n_points, finite coordinates with |x| <= 2^60";
  });
}

}  // extern "C"
