// abi_scan_prep.inl — C ABI: icp_scans_prepare_many, the aligned and partial targets of many raw scans (kernels_scan_prep.hip; the step
// apps/femur/AlignShapes.scala:30-55 and apps/bfm/AlignShapes.scala:33-101 start with).
//
// Item b: its points and landmarks under the caller's transform, the cuts around landmarks (the cut_count vertices smallest in
// (d², id): equal distances go to the lowest ids), the flag bytes, and the compaction of what no cut and no mask id took
// (maskPoints(...).transformedMesh [SCALISMO-UNVERIFIED]).  Every limit is checked for every item before the device is touched.  The
// items go through ONE buffer in rounds of at most kScanRoundWords 8-byte words (an item above that has a round of its own), in four
// regions: the bytes to be zeroed in front (flags, used), the inputs, the work arrays, the outputs — of which what depends on the
// counts (counts, kept ids, partial triangles and points) comes back through a host block, because only the host knows how many rows
// the caller's arrays get.  A round of small items (at most kScanPackWords of input and of output an item on average) packs its
// inputs into ONE upload and fetches its outputs as ONE copy each for the output and the flag regions: at femur size the eight
// copies an item would take cost more than everything else.  Per round: one fill, the uploads, seven launches, the copies back, ONE
// synchronisation.  It takes no context: a stream and buffers
// from the pools, as icp_gp_models_many.  An item's bits depend neither on the other items, nor on their order, nor on the rounds.

namespace {
constexpr size_t kScanRoundWords = (size_t)ICP_SCAN_PREP_ROUND_BYTES / sizeof(double);
constexpr size_t kScanPackWords = (size_t)32 << 10;  // 256 KiB
constexpr int kScanMaxPoints = 1 << 26;
constexpr double kScanMaxMagnitude = 0x1p400;
static_assert(kScanMaxCuts == ICP_SCAN_MAX_CUTS, "header and kernels agree on the cuts per item");

size_t scan_words(size_t bytes) { return (bytes + 7) / 8; }

// where an item's arrays lie, in 8-byte words from the start of its part of the round's region: zeroed bytes, inputs, work arrays,
// outputs (`counts` and what follows it: the late block, which depends on the counts)
struct ScanLayout {
  size_t zero_words, in_words, work_words, out_words;
  size_t flags, used;                                   // zeroed region
  size_t pts, lms, tris, mask;                          // inputs
  size_t keys, thr, keep, vpre, tpre, vblk, tblk;       // work arrays
  size_t aligned, lm_out, counts, kept, ptris, ppts;    // outputs
  ScanLayout(size_t M, size_t T, size_t L, size_t n_cuts, size_t n_mask) {
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += scan_words(bytes); return o; };
    flags = take(M); used = take(M);
    zero_words = at; at = 0;
    pts = take(24 * M); lms = take(24 * L); tris = take(12 * T); mask = take(4 * n_mask);
    in_words = at; at = 0;
    keys = take(8 * n_cuts * M); thr = take(16 * n_cuts); keep = take(T); vpre = take(4 * M); tpre = take(4 * T);
    vblk = take(4 * ((M + kScanTile - 1) / kScanTile)); tblk = take(4 * ((T + kScanTile - 1) / kScanTile));
    work_words = at; at = 0;
    aligned = take(24 * M); lm_out = take(24 * L); counts = take(8); kept = take(4 * M); ptris = take(12 * T); ppts = take(24 * M);
    out_words = at;
  }
  size_t words() const { return zero_words + in_words + work_words + out_words; }
  size_t late_words() const { return out_words - counts; }
};

bool scan_small(const double* v, size_t n) {  // finite and at most 2^400 in magnitude
  for (size_t i = 0; i < n; ++i)
    if (!(std::fabs(v[i]) <= kScanMaxMagnitude)) return false;
  return true;
}
bool scan_small_scaled(double s, const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!(std::fabs(s * v[i]) <= kScanMaxMagnitude)) return false;
  return true;
}
}  // namespace

extern "C" {

int icp_scans_prepare_many(int32_t n_items, int device, const int32_t* n_points, const double* const* points, const int32_t* n_triangles,
                           const int32_t* const* triangles, const icp_scan_transform* transforms, const int32_t* n_landmarks,
                           const double* const* landmarks, const int32_t* n_cuts, const int32_t* const* cut_landmark,
                           const int32_t* const* cut_count, const int32_t* n_mask_ids, const int32_t* const* mask_ids,
                           double* const* aligned_out, double* const* landmarks_out, uint8_t* const* cut_flags_out,
                           double* const* partial_points_out, int32_t* const* partial_triangles_out, int32_t* const* kept_ids_out,
                           int32_t* counts_out, int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(n_points && points && n_triangles && transforms && n_landmarks && n_cuts && n_mask_ids && status, "null argument");
    const int B = n_items;
    // ---- validation, item by item, before the device is touched
    item_status.assign(B, ICP_OK);
    std::vector<int> live;
    for (int b = 0; b < B; ++b) {
      auto good = [&] {
        const long long M = n_points[b], T = n_triangles[b], L = n_landmarks[b], nc = n_cuts[b], nm = n_mask_ids[b];
        if (M < 1 || M > kScanMaxPoints || T < 0 || T > kScanMaxPoints || L < 0 || nc < 0 || nc > kScanMaxCuts || nm < 0) return false;
        if (!points[b] || (T > 0 && !(triangles && triangles[b])) || (L > 0 && !(landmarks && landmarks[b]))) return false;
        if (nc > 0 && !(cut_landmark && cut_landmark[b] && cut_count && cut_count[b])) return false;
        if (nm > 0 && !(mask_ids && mask_ids[b])) return false;
        const icp_scan_transform& tf = transforms[b];
        if (tf.struct_size != sizeof(icp_scan_transform)) return false;
        if (!(std::isfinite(tf.pre_scale) && tf.pre_scale > 0.0)) return false;
        if (!scan_small(tf.rotation, 9) || !scan_small(tf.centre, 3) || !scan_small(tf.translation, 3)) return false;
        if (!scan_small(points[b], 3 * (size_t)M) || !scan_small_scaled(tf.pre_scale, points[b], 3 * (size_t)M)) return false;
        if (L > 0 && (!scan_small(landmarks[b], 3 * (size_t)L) || !scan_small_scaled(tf.pre_scale, landmarks[b], 3 * (size_t)L))) return false;
        for (long long i = 0; i < 3 * T; ++i)
          if (triangles[b][i] < 0 || triangles[b][i] >= M) return false;
        for (int j = 0; j < nc; ++j)
          if (cut_landmark[b][j] < 0 || cut_landmark[b][j] >= L || cut_count[b][j] < 0) return false;
        for (long long i = 0; i < nm; ++i)
          if (mask_ids[b][i] < 0) return false;
        return true;
      };
      if (good()) live.push_back(b);
      else item_status[b] = ICP_ERR_INVALID_ARG;
    }
    const int n_live = (int)live.size();
    if (n_live == 0) return;

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
      fail(ICP_ERR_DEVICE, std::string("no usable HIP device (this library has no CPU fallback): ") + hipGetErrorString(e));
    if (device < 0) {
      const char* lr = std::getenv("LOCAL_RANK");
      device = lr ? std::atoi(lr) % ndev : 0;
    }
    require(device < ndev, "device ordinal out of range");
    DeviceScope _dev(device);
    StreamScope _st(device);
    hipStream_t st = _st.st;

    // ---- the plan: every item's layout; rounds = ranges of consecutive live items whose footprints fit the budget
    const size_t cap = test_chunk_doubles("ICP_TEST_SCAN_PREP_CHUNK_DOUBLES", kScanRoundWords);
    struct Round { int q0, q1; size_t zero_words, in_words, work_words, out_words; };
    std::vector<ScanLayout> lay;
    std::vector<Round> rounds;
    lay.reserve(n_live);
    size_t buffer_words = 1, stage_in_words = 1, stage_out_words = 1, stage_zero_words = 1;
    {
      size_t used = 0;
      for (int q = 0; q < n_live; ++q) {
        const int b = live[q];
        lay.emplace_back((size_t)n_points[b], (size_t)n_triangles[b], (size_t)n_landmarks[b], (size_t)n_cuts[b], (size_t)n_mask_ids[b]);
        const ScanLayout& l = lay.back();
        if (rounds.empty() || used + l.words() > cap) {  // (an item above the budget: a round of its own)
          rounds.push_back(Round{q, q, 0, 0, 0, 0});
          used = 0;
        }
        Round& rd = rounds.back();
        rd.q1 = q + 1;
        rd.zero_words += l.zero_words; rd.in_words += l.in_words; rd.work_words += l.work_words; rd.out_words += l.out_words;
        used += l.words();
        buffer_words = std::max(buffer_words, used);
        stage_in_words = std::max(stage_in_words, rd.in_words);
        stage_out_words = std::max(stage_out_words, rd.out_words);
        stage_zero_words = std::max(stage_zero_words, rd.zero_words);
      }
    }
    DBuf<double> chunk;
    DBuf<ScanItem> d_items;
    std::vector<ScanItem> h_items(n_live);
    std::vector<size_t> zero_at(n_live), in_at(n_live), out_at(n_live);  // an item's parts, from the start of its round's regions
    chunk.alloc(buffer_words);
    for (const Round& rd : rounds) {
      size_t z = 0, in = 0, w = 0, o = 0;
      for (int q = rd.q0; q < rd.q1; ++q) {
        const int b = live[q];
        const ScanLayout& l = lay[q];
        const icp_scan_transform& tf = transforms[b];
        ScanItem& it = h_items[q];
        it = ScanItem{};
        it.M = n_points[b]; it.T = n_triangles[b]; it.L = n_landmarks[b]; it.n_cuts = n_cuts[b]; it.n_mask = n_mask_ids[b];
        for (int j = 0; j < it.n_cuts; ++j) {
          it.cut_landmark[j] = cut_landmark[b][j];
          it.cut_count[j] = std::min(cut_count[b][j], n_points[b]);
        }
        it.s = tf.pre_scale;
        std::memcpy(it.R, tf.rotation, sizeof(it.R));
        for (int d = 0; d < 3; ++d) {
          it.c[d] = tf.centre[d];
          it.o[d] = tf.centre[d] + tf.translation[d];
        }
        double* zb = chunk.p + z;
        double* ib = chunk.p + rd.zero_words + in;
        double* wb = chunk.p + rd.zero_words + rd.in_words + w;
        double* ob = chunk.p + rd.zero_words + rd.in_words + rd.work_words + o;
        it.flags = (unsigned char*)(zb + l.flags); it.used = (unsigned char*)(zb + l.used);
        it.pts = ib + l.pts; it.lms = ib + l.lms; it.tris = (const int*)(ib + l.tris); it.mask = (const int*)(ib + l.mask);
        it.keys = (unsigned long long*)(wb + l.keys); it.thr = (unsigned long long*)(wb + l.thr);
        it.keep = (unsigned char*)(wb + l.keep); it.vpre = (int*)(wb + l.vpre); it.tpre = (int*)(wb + l.tpre);
        it.vblk = (int*)(wb + l.vblk); it.tblk = (int*)(wb + l.tblk);
        it.aligned = ob + l.aligned; it.lm_out = ob + l.lm_out;
        it.counts = (int*)(ob + l.counts); it.kept = (int*)(ob + l.kept); it.ptris = (int*)(ob + l.ptris); it.ppts = ob + l.ppts;
        zero_at[q] = z; in_at[q] = in; out_at[q] = o;
        z += l.zero_words; in += l.in_words; w += l.work_words; o += l.out_words;
      }
    }
    {
      NullStreamBatch _nb;
      d_items.upload(h_items.data(), h_items.size());
    }
    std::vector<double> stage_in, stage_zero, stage_out(stage_out_words);
    const bool direct_only = dev_env("ICP_TEST_SCAN_PREP_DIRECT_COPIES") != nullptr;  // test-hooks build: small items take the large ones' copies

    // ---- the rounds
    for (const Round& rd : rounds) {
      const int n = rd.q1 - rd.q0;
      double* in_dev = chunk.p + rd.zero_words;
      double* out_dev = chunk.p + rd.zero_words + rd.in_words + rd.work_words;
      const bool packed = !direct_only && rd.in_words <= kScanPackWords * (size_t)n && rd.out_words <= kScanPackWords * (size_t)n;
      auto wants_late = [&](int b) {
        return counts_out || (partial_points_out && partial_points_out[b]) || (partial_triangles_out && partial_triangles_out[b]) ||
               (kept_ids_out && kept_ids_out[b]);
      };
      long long work_max = 0;
      int m_max = 0, t_max = 0;
      bool any_flags = false;
      for (int q = rd.q0; q < rd.q1; ++q) {
        const ScanItem& it = h_items[q];
        work_max = std::max(work_max, (long long)it.M + it.L + it.n_mask);
        m_max = std::max(m_max, it.M); t_max = std::max(t_max, it.T);
        any_flags = any_flags || (cut_flags_out && cut_flags_out[live[q]]);
      }
      HIP_OK(hipMemsetAsync(chunk.p, 0, sizeof(double) * rd.zero_words, st));
      HostCopies up, back;
      if (packed) {
        stage_in.resize(stage_in_words);
        for (int q = rd.q0; q < rd.q1; ++q) {
          const int b = live[q];
          const ScanItem& it = h_items[q];
          const ScanLayout& l = lay[q];
          double* blk = stage_in.data() + in_at[q];
          std::memcpy(blk + l.pts, points[b], sizeof(double) * 3 * (size_t)it.M);
          if (it.L > 0) std::memcpy(blk + l.lms, landmarks[b], sizeof(double) * 3 * (size_t)it.L);
          if (it.T > 0) std::memcpy(blk + l.tris, triangles[b], sizeof(int) * 3 * (size_t)it.T);
          if (it.n_mask > 0) std::memcpy(blk + l.mask, mask_ids[b], sizeof(int) * (size_t)it.n_mask);
        }
        up.add(in_dev, stage_in.data(), rd.in_words);
        up.issue(st, true);
      } else {
        for (int q = rd.q0; q < rd.q1; ++q) {
          const int b = live[q];
          const ScanItem& it = h_items[q];
          up.add(const_cast<double*>(it.pts), points[b], 3 * (size_t)it.M);
          if (it.L > 0) up.add(const_cast<double*>(it.lms), landmarks[b], 3 * (size_t)it.L);
        }
        up.issue(st, true);
        for (int q = rd.q0; q < rd.q1; ++q) {  // (the id arrays: counts of 4-byte words, copied as they are)
          const int b = live[q];
          const ScanItem& it = h_items[q];
          if (it.T > 0) HIP_OK(hipMemcpyAsync(const_cast<int*>(it.tris), triangles[b], sizeof(int) * 3 * (size_t)it.T, hipMemcpyHostToDevice, st));
          if (it.n_mask > 0) HIP_OK(hipMemcpyAsync(const_cast<int*>(it.mask), mask_ids[b], sizeof(int) * (size_t)it.n_mask, hipMemcpyHostToDevice, st));
        }
      }
      const ScanItem* items = d_items.p + rd.q0;
      launch_scan_transform(st, n, work_max, items);
      launch_scan_select(st, n, items);
      launch_scan_flags(st, n, m_max, items);
      launch_scan_triangles(st, n, t_max, items);
      launch_scan_prefix(st, n, std::max(m_max, t_max), items);
      launch_scan_scatter(st, n, std::max(m_max, t_max), items);
      if (packed) {
        back.add(out_dev, stage_out.data(), rd.out_words);
        if (any_flags) {
          stage_zero.resize(stage_zero_words);
          back.add(chunk.p, stage_zero.data(), rd.zero_words);
        }
        back.issue(st, false);
      } else {
        for (int q = rd.q0; q < rd.q1; ++q) {
          const int b = live[q];
          const ScanItem& it = h_items[q];
          const ScanLayout& l = lay[q];
          if (aligned_out && aligned_out[b]) back.add(it.aligned, aligned_out[b], 3 * (size_t)it.M);
          if (it.L > 0 && landmarks_out && landmarks_out[b]) back.add(it.lm_out, landmarks_out[b], 3 * (size_t)it.L);
          if (wants_late(b)) back.add(out_dev + out_at[q] + l.counts, stage_out.data() + out_at[q] + l.counts, l.late_words());
        }
        back.issue(st, false);
        for (int q = rd.q0; q < rd.q1; ++q) {
          const int b = live[q];
          if (cut_flags_out && cut_flags_out[b])
            HIP_OK(hipMemcpyAsync(cut_flags_out[b], h_items[q].flags, (size_t)h_items[q].M, hipMemcpyDeviceToHost, st));
        }
      }
      HIP_OK(hipStreamSynchronize(st));  // the round's one synchronisation
      for (int q = rd.q0; q < rd.q1; ++q) {
        const int b = live[q];
        const ScanLayout& l = lay[q];
        const ScanItem& it = h_items[q];
        const double* blk = stage_out.data() + out_at[q];
        if (packed) {
          if (aligned_out && aligned_out[b]) std::memcpy(aligned_out[b], blk + l.aligned, sizeof(double) * 3 * (size_t)it.M);
          if (it.L > 0 && landmarks_out && landmarks_out[b]) std::memcpy(landmarks_out[b], blk + l.lm_out, sizeof(double) * 3 * (size_t)it.L);
          if (cut_flags_out && cut_flags_out[b]) std::memcpy(cut_flags_out[b], stage_zero.data() + zero_at[q] + l.flags, (size_t)it.M);
        }
        if (!wants_late(b)) continue;
        int cnt[2];
        std::memcpy(cnt, blk + l.counts, sizeof(cnt));
        if (cnt[0] < 0 || cnt[0] > n_points[b] || cnt[1] < 0 || cnt[1] > n_triangles[b]) fail(ICP_ERR_DEVICE, "the compaction's counts are out of range");
        if (counts_out) { counts_out[2 * b] = cnt[0]; counts_out[2 * b + 1] = cnt[1]; }
        if (kept_ids_out && kept_ids_out[b]) std::memcpy(kept_ids_out[b], blk + l.kept, sizeof(int) * (size_t)cnt[0]);
        if (partial_triangles_out && partial_triangles_out[b]) std::memcpy(partial_triangles_out[b], blk + l.ptris, sizeof(int) * 3 * (size_t)cnt[1]);
        if (partial_points_out && partial_points_out[b]) std::memcpy(partial_points_out[b], blk + l.ppts, sizeof(double) * 3 * (size_t)cnt[0]);
      }
    }
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int) {
    return "an item is outside the limits: 1 <= n_points <= 2^26, 0 <= n_triangles <= 2^26 with ids in [0, n_points), struct_size, "
           "pre_scale > 0, finite values with |s*x|, |c|, |t|, |R_ij| <= 2^400, 0 <= n_cuts <= 7, 0 <= cut_landmark < n_landmarks, "
           "cut_count >= 0, mask ids >= 0";
  });
}

}  // extern "C"
