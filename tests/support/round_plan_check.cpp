// Stand-alone check (host compiler, no GPU, no HIP) of icp_round_plan.hpp: RegionCursor, RegionRounds<K> and RowPieces, the index
// arithmetic that decides which addresses the kernels of the context-free "many in one call" entry points get.
//
// The references are the loops these entry points were written with before they shared the header, restated as they stood: the
// `take` lambda of the layouts, the round accumulation and the per-item offsets of icp_scans_prepare_many (four regions),
// icp_decimate_many (three, and the most items of a round) and icp_surface_samples_many (three), and the piece loop of gpm_mspace_run
// (icp_nystrom_models_many had the same one).  Every integer the planners produce is compared with them: rounds, per-region totals,
// per-item offsets, buffer and staging sizes, pieces and where the flushes fall.  Exact comparisons, designed cases first, then random
// plans from a fixed seed.  Built and run by tests/test_round_plan_cpu.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../icp-proposal_amd/csrc/icp_round_plan.hpp"

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  size_t below(size_t n) { return (size_t)(next() % n); }
  bool chance(int percent) { return (int)(next() % 100) < percent; }
};

int g_failures = 0;
void expect(bool ok, const char* what, const char* name, long long a = 0, long long b = 0) {
  if (ok) return;
  if (++g_failures <= 20) std::printf("FAIL %s: %s (%lld vs %lld)\n", name, what, a, b);
}

// ---------------------------------------------------------------------------------------------------------------- the cursor
size_t ref_words(size_t bytes) { return (bytes + 7) / 8; }

void check_cursor(Rng& rng) {
  for (int trial = 0; trial < 2000; ++trial) {
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += ref_words(bytes); return o; };
    icp::RegionCursor c;
    for (int region = 0; region < 4; ++region) {
      const int n = (int)rng.below(8);
      for (int i = 0; i < n; ++i) {
        const size_t bytes = rng.chance(20) ? 0 : rng.below(rng.chance(50) ? 40 : 100000);
        const size_t a = take(bytes), b = c.take(bytes);
        expect(a == b, "an array's place", "cursor", (long long)a, (long long)b);
      }
      const size_t len = at;
      at = 0;
      const size_t got = c.close();
      expect(len == got, "a region's length", "cursor", (long long)len, (long long)got);
    }
  }
  expect(icp::region_words(0) == 0 && icp::region_words(1) == 1 && icp::region_words(8) == 1 && icp::region_words(9) == 2, "words of bytes",
         "cursor");
}

// ------------------------------------------------------------------------------------------------------------ region rounds
struct Lay4 { size_t zero_words, in_words, work_words, out_words; size_t words() const { return zero_words + in_words + work_words + out_words; } };
struct Lay3 { size_t in_words, work_words, out_words; size_t words() const { return in_words + work_words + out_words; } };

struct RefPlan {  // what the loops produce; regions in buffer order (a plan of three leaves the last column unused)
  struct Round { int q0, q1; size_t words[4]; };
  std::vector<Round> rounds;
  std::vector<std::vector<size_t>> at;  // [item][region]; -1 where the loops kept no offset
  size_t buffer_words = 0;
  long long stage[4] = {-1, -1, -1, -1};  // -1: the loops kept no such size
  int round_items = -1;
};

// icp_scans_prepare_many: zeroed, inputs, work, outputs
RefPlan ref_scan(const std::vector<Lay4>& lay_in, size_t cap) {
  const int n_live = (int)lay_in.size();
  struct Round { int q0, q1; size_t zero_words, in_words, work_words, out_words; };
  std::vector<Lay4> lay;
  std::vector<Round> rounds;
  size_t buffer_words = 1, stage_in_words = 1, stage_out_words = 1, stage_zero_words = 1;
  {
    size_t used = 0;
    for (int q = 0; q < n_live; ++q) {
      lay.push_back(lay_in[q]);
      const Lay4& l = lay.back();
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
  std::vector<size_t> zero_at(n_live), in_at(n_live), out_at(n_live), work_at(n_live);
  for (const Round& rd : rounds) {
    size_t z = 0, in = 0, w = 0, o = 0;
    for (int q = rd.q0; q < rd.q1; ++q) {
      const Lay4& l = lay[q];
      zero_at[q] = z; in_at[q] = in; out_at[q] = o;
      work_at[q] = w;  // (the loop used w for the work arrays' addresses: chunk.p + rd.zero_words + rd.in_words + w)
      z += l.zero_words; in += l.in_words; w += l.work_words; o += l.out_words;
    }
  }
  RefPlan r;
  for (const Round& rd : rounds) r.rounds.push_back(RefPlan::Round{rd.q0, rd.q1, {rd.zero_words, rd.in_words, rd.work_words, rd.out_words}});
  for (int q = 0; q < n_live; ++q) r.at.push_back({zero_at[q], in_at[q], work_at[q], out_at[q]});
  r.buffer_words = buffer_words;
  r.stage[0] = (long long)stage_zero_words; r.stage[1] = (long long)stage_in_words; r.stage[3] = (long long)stage_out_words;
  return r;
}

// icp_decimate_many: inputs, work, outputs; the most items of a round
RefPlan ref_decimate(const std::vector<Lay3>& lay_in, size_t cap) {
  const int n_live = (int)lay_in.size();
  struct Round { int q0, q1; size_t in_words, work_words, out_words; };
  std::vector<Lay3> lay;
  std::vector<Round> rounds;
  size_t buffer_words = 1, stage_in_words = 1, stage_out_words = 1;
  int round_items = 1;
  {
    size_t used = 0;
    for (int q = 0; q < n_live; ++q) {
      lay.push_back(lay_in[q]);
      const Lay3& l = lay.back();
      if (rounds.empty() || used + l.words() > cap) {  // (an item above the budget: a round of its own)
        rounds.push_back(Round{q, q, 0, 0, 0});
        used = 0;
      }
      Round& rd = rounds.back();
      rd.q1 = q + 1;
      rd.in_words += l.in_words; rd.work_words += l.work_words; rd.out_words += l.out_words;
      used += l.words();
      buffer_words = std::max(buffer_words, used);
      stage_in_words = std::max(stage_in_words, rd.in_words);
      stage_out_words = std::max(stage_out_words, rd.out_words);
      round_items = std::max(round_items, rd.q1 - rd.q0);
    }
  }
  std::vector<size_t> in_at(n_live), out_at(n_live), work_at(n_live);
  for (const Round& rd : rounds) {
    size_t in = 0, w = 0, o = 0;
    for (int q = rd.q0; q < rd.q1; ++q) {
      const Lay3& l = lay[q];
      in_at[q] = in; out_at[q] = o;
      work_at[q] = w;  // (chunk.p + rd.in_words + w)
      in += l.in_words; w += l.work_words; o += l.out_words;
    }
  }
  RefPlan r;
  for (const Round& rd : rounds) r.rounds.push_back(RefPlan::Round{rd.q0, rd.q1, {rd.in_words, rd.work_words, rd.out_words, 0}});
  for (int q = 0; q < n_live; ++q) r.at.push_back({in_at[q], work_at[q], out_at[q]});
  r.buffer_words = buffer_words;
  r.stage[0] = (long long)stage_in_words; r.stage[2] = (long long)stage_out_words;
  r.round_items = round_items;
  return r;
}

// icp_surface_samples_many: inputs, work, outputs
RefPlan ref_samples(const std::vector<Lay3>& lay_in, size_t cap) {
  const int n_live = (int)lay_in.size();
  struct Round { int q0, q1; size_t in_words, work_words, out_words; };
  std::vector<Lay3> lay;
  std::vector<Round> rounds;
  size_t buffer_words = 1, stage_in_words = 1, stage_out_words = 1;
  {
    size_t used = 0;
    for (int q = 0; q < n_live; ++q) {
      lay.push_back(lay_in[q]);
      const Lay3& l = lay.back();
      if (rounds.empty() || used + l.words() > cap) {  // (an item above the budget: a round of its own)
        rounds.push_back(Round{q, q, 0, 0, 0});
        used = 0;
      }
      Round& rd = rounds.back();
      rd.q1 = q + 1;
      rd.in_words += l.in_words; rd.work_words += l.work_words; rd.out_words += l.out_words;
      used += l.words();
      buffer_words = std::max(buffer_words, used);
      stage_in_words = std::max(stage_in_words, rd.in_words);
      stage_out_words = std::max(stage_out_words, rd.out_words);
    }
  }
  std::vector<size_t> in_at(n_live), out_at(n_live), work_at(n_live);
  for (const Round& rd : rounds) {
    size_t in = 0, w = 0, o = 0;
    for (int q = rd.q0; q < rd.q1; ++q) {
      const Lay3& l = lay[q];
      in_at[q] = in; out_at[q] = o;
      work_at[q] = w;  // (chunk.p + rd.in_words + w)
      in += l.in_words; w += l.work_words; o += l.out_words;
    }
  }
  RefPlan r;
  for (const Round& rd : rounds) r.rounds.push_back(RefPlan::Round{rd.q0, rd.q1, {rd.in_words, rd.work_words, rd.out_words, 0}});
  for (int q = 0; q < n_live; ++q) r.at.push_back({in_at[q], work_at[q], out_at[q]});
  r.buffer_words = buffer_words;
  r.stage[0] = (long long)stage_in_words; r.stage[2] = (long long)stage_out_words;
  return r;
}

template <int K>
void compare(const icp::RegionRounds<K>& plan, const RefPlan& ref, const char* name) {
  expect(plan.rounds.size() == ref.rounds.size(), "the number of rounds", name, (long long)plan.rounds.size(), (long long)ref.rounds.size());
  expect(plan.at.size() == ref.at.size(), "the number of items", name, (long long)plan.at.size(), (long long)ref.at.size());
  if (plan.rounds.size() != ref.rounds.size() || plan.at.size() != ref.at.size()) return;
  for (size_t i = 0; i < ref.rounds.size(); ++i) {
    const auto& a = plan.rounds[i];
    const RefPlan::Round& b = ref.rounds[i];
    expect(a.q0 == b.q0 && a.q1 == b.q1, "a round's items", name, a.q0, b.q0);
    size_t base = 0;
    for (int k = 0; k < K; ++k) {
      expect(a.words[k] == b.words[k], "a region's total", name, (long long)a.words[k], (long long)b.words[k]);
      expect(a.base(k) == base, "a region's start: the regions lie in index order", name, (long long)a.base(k), (long long)base);
      base += b.words[k];
    }
  }
  for (size_t q = 0; q < ref.at.size(); ++q)
    for (int k = 0; k < K; ++k) expect(plan.at[q][k] == ref.at[q][k], "an item's offset", name, (long long)plan.at[q][k], (long long)ref.at[q][k]);
  expect(plan.buffer_words == ref.buffer_words, "buffer_words", name, (long long)plan.buffer_words, (long long)ref.buffer_words);
  for (int k = 0; k < K; ++k) {
    expect(plan.stage_words[k] >= 1, "a staging size of at least 1", name, (long long)plan.stage_words[k]);
    if (ref.stage[k] >= 0) expect((long long)plan.stage_words[k] == ref.stage[k], "a staging size", name, (long long)plan.stage_words[k], ref.stage[k]);
  }
  if (ref.round_items >= 0) expect(plan.round_items == ref.round_items, "the most items of a round", name, plan.round_items, ref.round_items);
}

void check_regions3(const std::vector<Lay3>& lay, size_t cap, const char* name) {
  icp::RegionRounds<3> plan(cap, lay.size());
  for (const Lay3& l : lay) {
    const size_t w[3] = {l.in_words, l.work_words, l.out_words};
    plan.add(w);
  }
  compare<3>(plan, ref_decimate(lay, cap), name);
  compare<3>(plan, ref_samples(lay, cap), name);
}
void check_regions4(const std::vector<Lay4>& lay, size_t cap, const char* name) {
  icp::RegionRounds<4> plan(cap, lay.size());
  for (const Lay4& l : lay) {
    const size_t w[4] = {l.zero_words, l.in_words, l.work_words, l.out_words};
    plan.add(w);
  }
  compare<4>(plan, ref_scan(lay, cap), name);
}
// one list of footprints under both region counts: an item of `total` words, split over the regions
void check_both(const std::vector<size_t>& totals, size_t cap, const char* name) {
  std::vector<Lay3> l3;
  std::vector<Lay4> l4;
  for (size_t t : totals) {
    const size_t a = t / 3, b = t / 5;
    l3.push_back(Lay3{a, b, t - a - b});
    const size_t z = t / 7;
    l4.push_back(Lay4{z, a, b, t - a - b - z});
  }
  check_regions3(l3, cap, name);
  check_regions4(l4, cap, name);
}

void check_regions(Rng& rng) {
  check_both({5}, 100, "one item");
  check_both({100}, 100, "one item of exactly cap");
  check_both({101}, 100, "one item of cap + 1");
  check_both({101, 100}, 100, "cap words behind an oversize round");
  check_both({40, 60}, 100, "an item that fills the round exactly stays in it");
  check_both({40, 100}, 100, "cap words behind a non-empty round");
  check_both({100, 100, 100}, 100, "cap words one after the other");
  check_both({40, 101, 40, 20}, 100, "cap + 1 between small items");
  check_both({1, 1, 1}, 1, "cap = 1");
  check_both({2, 1, 3}, 1, "cap = 1 with oversize items");
  check_both({150, 101, 1000, 102}, 100, "every item oversize");
  check_both({}, 100, "no item");
  {
    // a region of length 0: T = 0 leaves decimate's triangle arrays empty; here whole regions
    check_regions3({Lay3{10, 0, 4}, Lay3{0, 0, 7}, Lay3{3, 0, 0}, Lay3{30, 0, 2}}, 40, "a region of length 0 (K = 3)");
    check_regions4({Lay4{0, 10, 0, 4}, Lay4{2, 0, 0, 7}, Lay4{0, 3, 5, 0}, Lay4{0, 30, 0, 2}}, 40, "a region of length 0 (K = 4)");
    check_regions3({Lay3{0, 0, 0}, Lay3{0, 0, 0}}, 1, "items without a word (K = 3)");
    check_regions4({Lay4{0, 0, 0, 0}}, 1, "an item without a word (K = 4)");
  }
  for (int trial = 0; trial < 4000; ++trial) {
    const size_t cap = 1 + rng.below(rng.chance(30) ? 8 : 600);
    const int n = (int)rng.below(40);
    const size_t span = rng.chance(50) ? cap : 2 * cap + 2;
    std::vector<Lay3> l3;
    std::vector<Lay4> l4;
    for (int q = 0; q < n; ++q) {
      auto part = [&]() -> size_t { return rng.chance(25) ? 0 : rng.below(span / 2 + 1); };
      l3.push_back(Lay3{part(), part(), part()});
      l4.push_back(Lay4{part() / 2, part(), part(), part() / 2});
      if (rng.chance(10)) {  // exactly what is left of the budget, or one word more
        l3.back() = Lay3{cap / 2, 0, cap - cap / 2 + (rng.chance(50) ? 1 : 0)};
        l4.back() = Lay4{0, cap / 2, cap - cap / 2 + (rng.chance(50) ? 1 : 0), 0};
      }
    }
    check_regions3(l3, cap, "random plan (K = 3)");
    check_regions4(l4, cap, "random plan (K = 4)");
  }
}

// ---------------------------------------------------------------------------------------------------------------- row pieces
struct PieceItem { int R, rank; bool basis; };
struct Piece { int item, row0, rows; size_t offset; };
struct PiecePlan {
  std::vector<Piece> pieces;
  std::vector<size_t> flushes;  // how many pieces had been made when a launch went out
};

// run_rounds of gpm_mspace_run; `flush` launches what `pcs` holds
PiecePlan ref_pieces(const std::vector<PieceItem>& items, size_t cap, int kGpmRowQuantum, int kGpmMaxPieces) {
  PiecePlan out;
  std::vector<Piece> pcs;
  size_t used = 0;
  auto flush = [&] {
    if (pcs.empty()) return;
    out.flushes.push_back(out.pieces.size());
    pcs.clear();
    used = 0;
  };
  for (int q = 0; q < (int)items.size(); ++q) {
    if (!items[q].basis) continue;
    const PieceItem& sp = items[q];
    const size_t per_q = (size_t)kGpmRowQuantum * sp.rank;
    for (int row0 = 0; row0 < sp.R;) {
      if (cap - used < per_q || (int)pcs.size() == kGpmMaxPieces) flush();
      const size_t fit = (cap - used) / per_q * kGpmRowQuantum;
      const int rows = (int)std::min<size_t>(fit, (size_t)(sp.R - row0));
      Piece pc{q, row0, rows, used};
      used += (size_t)rows * sp.rank;
      pcs.push_back(pc);
      out.pieces.push_back(pc);
      row0 += rows;
    }
  }
  flush();
  return out;
}

void check_pieces_case(const std::vector<PieceItem>& items, size_t cap, int quantum, int max_pieces, const char* name) {
  const PiecePlan ref = ref_pieces(items, cap, quantum, max_pieces);
  PiecePlan got;
  icp::RowPieces{cap, quantum, max_pieces}.cut(
      0, (int)items.size(), [&](int q) { return icp::RowPieces::Item{items[q].R, (size_t)items[q].rank, items[q].basis}; },
      [&](int q, int row0, int rows, size_t offset) { got.pieces.push_back(Piece{q, row0, rows, offset}); },
      [&] { got.flushes.push_back(got.pieces.size()); });
  expect(got.pieces.size() == ref.pieces.size(), "the number of pieces", name, (long long)got.pieces.size(), (long long)ref.pieces.size());
  expect(got.flushes == ref.flushes, "where the flushes fall", name, (long long)got.flushes.size(), (long long)ref.flushes.size());
  if (got.pieces.size() != ref.pieces.size()) return;
  for (size_t i = 0; i < ref.pieces.size(); ++i) {
    const Piece &a = got.pieces[i], &b = ref.pieces[i];
    expect(a.item == b.item && a.row0 == b.row0 && a.rows == b.rows && a.offset == b.offset, "a piece", name, a.row0, b.row0);
    expect(a.rows > 0 && a.offset + (size_t)a.rows * items[a.item].rank <= cap, "a piece lies inside the chunk", name, (long long)a.offset);
  }
  // every row of every item that takes part, once and in order
  size_t i = 0;
  for (int q = 0; q < (int)items.size(); ++q) {
    if (!items[q].basis) continue;
    int row = 0;
    for (; i < got.pieces.size() && got.pieces[i].item == q; ++i) {
      expect(got.pieces[i].row0 == row, "an item's pieces follow each other", name, got.pieces[i].row0, row);
      row += got.pieces[i].rows;
    }
    expect(row == items[q].R, "an item's rows are all cut", name, row, items[q].R);
  }
  expect(i == got.pieces.size(), "no piece of an item that takes no part", name);
}

void check_pieces(Rng& rng) {
  check_pieces_case({{30, 4, true}}, 1000, 48, 32768, "R < 48");
  check_pieces_case({{100, 4, true}}, 48 * 4, 48, 32768, "R no multiple of 48, cap == per_q");
  check_pieces_case({{500, 3, true}, {7, 3, true}, {96, 3, true}}, 48 * 3, 48, 32768, "cap == per_q: a piece always fits");
  check_pieces_case({{500, 5, true}, {301, 2, true}}, 48 * 5 * 2 + 77, 48, 32768, "a per_q that does not divide cap");
  check_pieces_case({{200, 4, true}, {300, 4, false}, {200, 4, true}}, 48 * 4 * 3, 48, 32768, "an item that takes no part between two that do");
  check_pieces_case({{10, 2, true}, {10, 2, true}, {10, 2, true}, {10, 2, true}, {10, 2, true}, {10, 2, true}, {10, 2, true}}, 100000, 48, 3,
                    "a piece cap of 3: the count-triggered flush");
  check_pieces_case({{480, 2, true}}, 48 * 2, 48, 3, "a piece cap of 3 under a full buffer");
  check_pieces_case({{0, 2, true}, {5, 1, false}}, 1000, 48, 3, "nothing to cut");
  check_pieces_case({}, 1000, 48, 3, "no item");
  for (int trial = 0; trial < 4000; ++trial) {
    const int quantum = rng.chance(70) ? 48 : 1 + (int)rng.below(64);
    const int n = (int)rng.below(12);
    std::vector<PieceItem> items;
    int rank_max = 1;
    for (int q = 0; q < n; ++q) {
      const int rank = 1 + (int)rng.below(rng.chance(50) ? 4 : 40);
      items.push_back(PieceItem{(int)rng.below(rng.chance(50) ? 100 : 3000), rank, !rng.chance(20)});
      rank_max = std::max(rank_max, rank);
    }
    // as the entry points size it: the hook's or the default chunk, and never less than a quantum of the widest item
    size_t cap = 1 + rng.below(rng.chance(50) ? 400 : 40000);
    cap = std::max(cap, (size_t)quantum * rank_max);
    const int max_pieces = rng.chance(30) ? 1 + (int)rng.below(5) : 32768;
    check_pieces_case(items, cap, quantum, max_pieces, "random plan");
  }
}

}  // namespace

int main() {
  Rng rng{0x9e3779b97f4a7c15ull};
  check_cursor(rng);
  check_regions(rng);
  check_pieces(rng);
  if (g_failures) {
    std::printf("%d failures\n", g_failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
