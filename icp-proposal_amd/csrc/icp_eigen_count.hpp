// icp_eigen_count.hpp — the count of a proposal's decompositions (plain C++: no HIP, no other header of the library; the
// stand-alone check of tests/test_eigen_count_cpu.py includes it as it is)
//
// Every 128th decomposition of a proposal starts cold, from the identity, which puts an end to the deviation from orthogonality
// that warm starts hand on (icp_proposal::prepare_eigen).  Which step a cold start falls on decides the chain's last bits, so the
// PLACE a decomposition takes in the cycle of 128 must not depend on when it is launched — lane 1 of a twin pass is decomposed
// before anybody knows whether it will be used, and gives its place back when it is not.  The NUMBER a launch raises its entry's
// completion word to (and its cancel slot is keyed by) is another matter: a dropped launch still raises the word, so a number is
// never handed out twice.  Hence two counters.
#pragma once

namespace icp {

struct EigenCount {
  static constexpr int kCycle = 128;
  int place = 0;   // places taken so far (the on-device loops carry this one through their chains)
  int number = 0;  // numbers issued so far: monotone, never given back
  struct Ticket { int number; bool cold; };
  // a decomposition started (or planned) ahead of its use: cold where it takes the first place of a cycle
  bool ahead_cold() const { return (place & (kCycle - 1)) == kCycle - 1; }
  Ticket take_ahead() { const bool cold = ahead_cold(); ++place; return Ticket{++number, cold}; }
  // a place without a launch (speculation switched off: icp_proposal::plan_eigen); the launch that uses it later takes issue()
  bool plan() { const bool cold = ahead_cold(); ++place; return cold; }
  int issue() { return ++number; }
  // the ordinary decomposition of a state on record (prepare_eigen): cold where the place it takes is the last of a cycle
  Ticket take_ordinary() { ++place; return Ticket{++number, ((place + 1) & (kCycle - 1)) == 0}; }
  // A place goes back: a lane 1 that is not used, a step that is repeated from scratch (its number stays spent).  The count is
  // only a count: if an ordinary decomposition took a place between lane 1's launch and its cancellation (a per-method call between
  // two chain steps), that one made its cold decision one place later than it would have one call at a time — the cycle stays 128
  // long, the cold start moves by one decomposition; chains stepped through icp_chain_step alone never do this.
  void give_back() { --place; }
  // A writer outside this count — the on-device loops, which carry `place` through their chains and raise the completion words of
  // the entries they decompose to the places they take — may have written words up to `highest`: no number at or below it is issued
  // any more (a waiter compares word - number >= 0: a number below a stale word would find its basis "complete" at once).
  void foreign_words_up_to(int highest) { if (number < highest) number = highest; }
};

}  // namespace icp
