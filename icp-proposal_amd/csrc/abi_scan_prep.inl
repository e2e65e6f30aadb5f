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
// synchronisation.  It takes no context: the live items, the device and the stream are abi_pool_many.inl's, the rounds and every
// item's place in their regions RegionRounds' (icp_round_plan.hpp).  An item's bits depend neither on the other items, nor on their
// order, nor on the rounds.

namespace {
constexpr size_t kScanRoundWords = (size_t)ICP_SCAN_PREP_ROUND_BYTES / sizeof(double);
constexpr size_t kScanPackWords = (size_t)32 << 10;  // 256 KiB
constexpr int kScanMaxPoints = 1 << 26;
constexpr double kScanMaxMagnitude = 0x1p400;
static_assert(kScanMaxCuts == ICP_SCAN_MAX_CUTS, "header and kernels agree on the cuts per item");

enum { kScanZero, kScanIn, kScanWork, kScanOut };  // the regions of a round's buffer, in their order

// where an item's arrays lie, in 8-byte words from the start of its part of the round's region: zeroed bytes, inputs, work arrays,
// outputs (`counts` and what follows it: the late block, which depends on the counts)
struct ScanLayout {
  size_t words[4];                                      // the regions' lengths
  size_t flags, used;                                   // zeroed region
  size_t pts, lms, tris, mask;                          // inputs
  size_t keys, thr, keep, vpre, tpre, vblk, tblk;       // work arrays
  size_t aligned, lm_out, counts, kept, ptris, ppts;    // outputs
  ScanLayout(size_t M, size_t T, size_t L, size_t n_cuts, size_t n_mask) {
    RegionCursor c;
    flags = c.take(M); used = c.take(M);
    words[kScanZero] = c.close();
    pts = c.take(24 * M); lms = c.take(24 * L); tris = c.take(12 * T); mask = c.take(4 * n_mask);
    words[kScanIn] = c.close();
    keys = c.take(8 * n_cuts * M); thr = c.take(16 * n_cuts); keep = c.take(T); vpre = c.take(4 * M); tpre = c.take(4 * T);
    vblk = c.take(4 * ((M + kScanTile - 1) / kScanTile)); tblk = c.take(4 * ((T + kScanTile - 1) / kScanTile));
    words[kScanWork] = c.close();
    aligned = c.take(24 * M); lm_out = c.take(24 * L); counts = c.take(8); kept = c.take(4 * M); ptris = c.take(12 * T); ppts = c.take(24 * M);
    words[kScanOut] = c.close();
  }
  size_t late_words() const { return words[kScanOut] - counts; }
};

bool scan_small(const double* v, size_t n) { return all_within(v, n, kScanMaxMagnitude); }  // finite and at most 2^400 in magnitude
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
    const std::vector<int> live = live_items(B, item_status, [&](int b) {
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
      if (T > 0 && !ids_in_range(triangles[b], 3 * (size_t)T, M)) return false;
      for (int j = 0; j < nc; ++j)
        if (cut_landmark[b][j] < 0 || cut_landmark[b][j] >= L || cut_count[b][j] < 0) return false;
      for (long long i = 0; i < nm; ++i)
        if (mask_ids[b][i] < 0) return false;
      return true;
    });
    const int n_live = (int)live.size();
    if (n_live == 0) return;

    PoolCall call(device);
    hipStream_t st = call.st;

    // ---- the plan: every item's layout; rounds = ranges of consecutive live items whose footprints fit the budget
    std::vector<ScanLayout> lay;
    lay.reserve(n_live);
    RegionRounds<4> plan(test_chunk_doubles("ICP_TEST_SCAN_PREP_CHUNK_DOUBLES", kScanRoundWords), n_live);
    using Round = RegionRounds<4>::Round;
    for (int b : live) {
      lay.emplace_back((size_t)n_points[b], (size_t)n_triangles[b], (size_t)n_landmarks[b], (size_t)n_cuts[b], (size_t)n_mask_ids[b]);
      plan.add(lay.back().words);
    }
    const size_t stage_zero_words = plan.stage_words[kScanZero], stage_in_words = plan.stage_words[kScanIn],
                 stage_out_words = plan.stage_words[kScanOut];
    DBuf<double> chunk;
    DBuf<ScanItem> d_items;
    std::vector<ScanItem> h_items(n_live);
    chunk.alloc(plan.buffer_words);
    for (const Round& rd : plan.rounds) {
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
        const auto& at = plan.at[q];  // the item's parts, from the start of its round's regions
        double* zb = chunk.p + rd.base(kScanZero) + at[kScanZero];
        double* ib = chunk.p + rd.base(kScanIn) + at[kScanIn];
        double* wb = chunk.p + rd.base(kScanWork) + at[kScanWork];
        double* ob = chunk.p + rd.base(kScanOut) + at[kScanOut];
        it.flags = (unsigned char*)(zb + l.flags); it.used = (unsigned char*)(zb + l.used);
        it.pts = ib + l.pts; it.lms = ib + l.lms; it.tris = (const int*)(ib + l.tris); it.mask = (const int*)(ib + l.mask);
        it.keys = (unsigned long long*)(wb + l.keys); it.thr = (unsigned long long*)(wb + l.thr);
        it.keep = (unsigned char*)(wb + l.keep); it.vpre = (int*)(wb + l.vpre); it.tpre = (int*)(wb + l.tpre);
        it.vblk = (int*)(wb + l.vblk); it.tblk = (int*)(wb + l.tblk);
        it.aligned = ob + l.aligned; it.lm_out = ob + l.lm_out;
        it.counts = (int*)(ob + l.counts); it.kept = (int*)(ob + l.kept); it.ptris = (int*)(ob + l.ptris); it.ppts = ob + l.ppts;
      }
    }
    {
      NullStreamBatch _nb;
      d_items.upload(h_items.data(), h_items.size());
    }
    std::vector<double> stage_in, stage_zero, stage_out(stage_out_words);
    const bool direct_only = dev_env("ICP_TEST_SCAN_PREP_DIRECT_COPIES") != nullptr;  // test-hooks build: small items take the large ones' copies

    // ---- the rounds
    for (const Round& rd : plan.rounds) {
      const int n = rd.q1 - rd.q0;
      const size_t zero_words = rd.words[kScanZero], in_words = rd.words[kScanIn], out_words = rd.words[kScanOut];
      double* in_dev = chunk.p + rd.base(kScanIn);
      double* out_dev = chunk.p + rd.base(kScanOut);
      const bool packed = !direct_only && in_words <= kScanPackWords * (size_t)n && out_words <= kScanPackWords * (size_t)n;
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
      HIP_OK(hipMemsetAsync(chunk.p, 0, sizeof(double) * zero_words, st));
      HostCopies up, back;
      if (packed) {
        stage_in.resize(stage_in_words);
        for (int q = rd.q0; q < rd.q1; ++q) {
          const int b = live[q];
          const ScanItem& it = h_items[q];
          const ScanLayout& l = lay[q];
          double* blk = stage_in.data() + plan.at[q][kScanIn];
          std::memcpy(blk + l.pts, points[b], sizeof(double) * 3 * (size_t)it.M);
          if (it.L > 0) std::memcpy(blk + l.lms, landmarks[b], sizeof(double) * 3 * (size_t)it.L);
          if (it.T > 0) std::memcpy(blk + l.tris, triangles[b], sizeof(int) * 3 * (size_t)it.T);
          if (it.n_mask > 0) std::memcpy(blk + l.mask, mask_ids[b], sizeof(int) * (size_t)it.n_mask);
        }
        up.add(in_dev, stage_in.data(), in_words);
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
        back.add(out_dev, stage_out.data(), out_words);
        if (any_flags) {
          stage_zero.resize(stage_zero_words);
          back.add(chunk.p, stage_zero.data(), zero_words);
        }
        back.issue(st, false);
      } else {
        for (int q = rd.q0; q < rd.q1; ++q) {
          const int b = live[q];
          const ScanItem& it = h_items[q];
          const ScanLayout& l = lay[q];
          if (aligned_out && aligned_out[b]) back.add(it.aligned, aligned_out[b], 3 * (size_t)it.M);
          if (it.L > 0 && landmarks_out && landmarks_out[b]) back.add(it.lm_out, landmarks_out[b], 3 * (size_t)it.L);
          if (wants_late(b)) back.add(out_dev + plan.at[q][kScanOut] + l.counts, stage_out.data() + plan.at[q][kScanOut] + l.counts, l.late_words());
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
        const double* blk = stage_out.data() + plan.at[q][kScanOut];
        if (packed) {
          if (aligned_out && aligned_out[b]) std::memcpy(aligned_out[b], blk + l.aligned, sizeof(double) * 3 * (size_t)it.M);
          if (it.L > 0 && landmarks_out && landmarks_out[b]) std::memcpy(landmarks_out[b], blk + l.lm_out, sizeof(double) * 3 * (size_t)it.L);
          if (cut_flags_out && cut_flags_out[b]) std::memcpy(cut_flags_out[b], stage_zero.data() + plan.at[q][kScanZero] + l.flags, (size_t)it.M);
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
