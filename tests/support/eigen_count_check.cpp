// Stand-alone check (host compiler, no GPU, no HIP) of icp::EigenCount, the count of a proposal's decompositions: the places in the
// cycle of 128 that decide cold starts, and the completion-word numbers.
//
// A random chain is played twice.  ONE AT A TIME: a single counter, as the library kept it while lane 1 of a twin pass was decomposed
// at its own call — a used lane 1 takes the place behind lane 0's, a dropped one none, a step repeated from scratch skips 127 places
// (a launched decomposition) or steps one back (a planned one).  EARLY: EigenCount, lane 1 decomposed together with lane 0 and its
// place given back where it is not used, a repeated step's places given back.  Every decomposition both orders have in common must
// start cold in the one exactly when it does in the other, and no number may be issued twice.
// Now and then a FOREIGN WRITER takes the count over, as the on-device loops do: it counts on from the place, raises completion words
// to the places it takes (one per accepted step) and hands the place back — or fails and hands nothing back.  No number issued
// afterwards may lie at or below a word it wrote: a waiter compares word - number >= 0.
// Built and run by tests/test_eigen_count_cpu.py.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "../../icp-proposal_amd/csrc/icp_eigen_count.hpp"

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  bool chance(int percent) { return (int)(next() % 100) < percent; }
};

// the single counter of the one-at-a-time order
struct Legacy {
  int seq = 0;
  bool ahead() { const bool cold = (seq & 127) == 127; ++seq; return cold; }     // speculate_eigen
  bool plan() { const bool cold = (seq & 127) == 127; ++seq; return cold; }      // plan_eigen
  bool ordinary() { ++seq; return ((seq + 1) & 127) == 0; }                      // prepare_eigen
  void withdraw_launched() { seq += 127; }
  void withdraw_planned() { --seq; }
};

struct Run {
  icp::EigenCount n;
  Legacy o;
  std::set<int> numbers;
  long compared = 0, cold = 0, lane1_cold = 0, given_back = 0, loops = 0, loops_ahead = 0;
  int highest_word = 0;  // … a foreign writer has raised
  bool ok = true;

  void number(int v) {
    if (!numbers.insert(v).second) { std::printf("number %d issued twice\n", v); ok = false; }
    if (v <= highest_word) { std::printf("number %d at or below a foreign word %d\n", v, highest_word); ok = false; }
  }
  // an on-device loop of n steps, `accepted` of them accepted; failed: it hands nothing back
  void foreign_loop(int n, int accepted, bool failed) {
    ++loops;
    loops_ahead += this->n.place + accepted > this->n.number;  // (without the cover below the next numbers would lie below its words)
    this->n.foreign_words_up_to(this->n.place + n);            // at the hand-over TO the loop: whatever becomes of it
    if (accepted > 0 && this->n.place + accepted > highest_word) highest_word = this->n.place + accepted;
    if (failed) return;
    for (int k = 0; k < accepted; ++k) {  // the loop's own cold rule is the ordinary one, on the carried place (k_mh_decide)
      ++this->n.place; ++o.seq;
      ++compared;
    }
  }
  void same(bool a, bool b, const char* what, long step) {
    ++compared;
    cold += a;
    if (a != b) { std::printf("step %ld, %s: cold %d one at a time, %d early\n", step, what, (int)a, (int)b); ok = false; }
  }
};

// one step of the chain (or two: a twin pass); planned: speculation switched off, places are planned instead of launched
void play(Run& r, Rng& g, long step, bool planned) {
  const bool twin = g.chance(45), withdrawn = g.chance(3), lane0_accepted = g.chance(33);
  if (g.chance(1)) {
    const int n = 1 + (int)(g.next() % 400);
    r.foreign_loop(n, (int)(g.next() % (unsigned)(n + 1)), g.chance(20));
  }
  if (g.chance(10)) {  // a state that reaches the record undecomposed: the ordinary decomposition
    const icp::EigenCount::Ticket t = r.n.take_ordinary();
    r.number(t.number);
    r.same(r.o.ordinary(), t.cold, "ordinary", step);
  }
  if (planned) {  // (lane 1 plans at its own call in either order)
    bool c_new = r.n.plan(), c_old = r.o.plan();
    r.same(c_old, c_new, "planned", step);
    if (withdrawn) {
      r.n.give_back(); r.o.withdraw_planned();
      c_new = r.n.plan(); c_old = r.o.plan();
      r.same(c_old, c_new, "planned again", step);
    }
    if (lane0_accepted) r.number(r.n.issue());  // (its launch, one step later)
    else if (twin) r.same(r.o.plan(), r.n.plan(), "planned lane 1", step);
    return;
  }
  // the call that finishes the pass: lane 0's decomposition — and, early, lane 1's
  icp::EigenCount::Ticket t0 = r.n.take_ahead();
  r.number(t0.number);
  bool c0_old = r.o.ahead();
  r.same(c0_old, t0.cold, "lane 0", step);
  icp::EigenCount::Ticket t1{0, false};
  if (twin) { t1 = r.n.take_ahead(); r.number(t1.number); }
  if (withdrawn) {  // the call is repeated from scratch, as a one-lane step: everything it started is withdrawn
    if (twin) r.n.give_back();
    r.n.give_back();
    r.o.withdraw_launched();
    t0 = r.n.take_ahead();
    r.number(t0.number);
    r.same(r.o.ahead(), t0.cold, "lane 0 again", step);
    return;
  }
  if (!twin) return;
  if (lane0_accepted) {  // lane 1 dropped: its place goes back, its number stays spent
    r.n.give_back();
    ++r.given_back;
    return;
  }
  // lane 0 rejected, lane 1's call: one at a time its decomposition goes out now
  bool c1_old = r.o.ahead();
  r.same(c1_old, t1.cold, "lane 1", step);
  r.lane1_cold += t1.cold;
  if (g.chance(3)) {  // lane 1's call is repeated from scratch
    r.n.give_back();
    r.o.withdraw_launched();
    t1 = r.n.take_ahead();
    r.number(t1.number);
    r.same(r.o.ahead(), t1.cold, "lane 1 again", step);
  }
}

}  // namespace

int main() {
  bool ok = true;
  for (uint64_t seed = 1; seed <= 8; ++seed) {
    Run r;
    Rng g{seed * 0x9E3779B97F4A7C15ull};
    for (long step = 0; step < 20000 && r.ok; ++step) play(r, g, step, /*planned=*/seed % 4 == 0 ? g.chance(50) : false);
    std::printf("seed %llu: %ld decompositions compared, %ld cold (%ld on a lane 1), %ld places given back, %zu numbers, places %d / %d\n",
                (unsigned long long)seed, r.compared, r.cold, r.lane1_cold, r.given_back, r.numbers.size(), r.n.place, r.o.seq);
    // (the two counts agree modulo the cycle: a withdrawn launch skips a whole cycle one at a time)
    if ((r.n.place - r.o.seq) % icp::EigenCount::kCycle != 0) { std::printf("places differ modulo the cycle\n"); r.ok = false; }
    std::printf("        %ld foreign loops, %ld of them past the numbers, highest word %d, numbers up to %d\n", r.loops, r.loops_ahead, r.highest_word,
                r.n.number);
    if (r.cold == 0 || r.lane1_cold == 0 || r.given_back == 0 || r.loops == 0 || r.loops_ahead == 0) { std::printf("the sequence exercised nothing\n"); r.ok = false; }
    ok = ok && r.ok;
  }
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
