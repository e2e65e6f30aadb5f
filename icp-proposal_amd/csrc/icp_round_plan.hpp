// icp_round_plan.hpp — the index arithmetic of the "many in one call" entry points that take a stream and buffers from the pools
// (plain C++: no HIP, no other header of the library; the stand-alone check of tests/test_round_plan_cpu.py includes it as it is)
//
// Two plans.  RegionRounds: items that go through ONE buffer in rounds, every round's buffer cut into K regions (inputs, work arrays,
// outputs, ...) that hold the parts of the round's items one behind the other — which decides the addresses the kernels get.
// RowPieces: rows of many items cut into pieces that fill a chunk buffer, a launch per filling.
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <vector>

namespace icp {

inline size_t region_words(size_t bytes) { return (bytes + 7) / 8; }

// the arrays of one item inside one region, in 8-byte words from the start of the item's part: take() gives an array's place, close()
// the part's length (and starts the next region at 0)
struct RegionCursor {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at += region_words(bytes);
    return o;
  }
  size_t close() {
    const size_t n = at;
    at = 0;
    return n;
  }
};

// Rounds = ranges of consecutive items whose footprints (the sum of their K region lengths) fit `cap` words; an item above the cap has
// a round of its own, and one that fills the round exactly stays in it.  A round's regions lie in the buffer in index order.
template <int K>
struct RegionRounds {
  struct Round {
    int q0, q1;       // items q0 .. q1-1
    size_t words[K];  // the regions' lengths
    size_t base(int k) const {  // where region k starts in the buffer
      size_t o = 0;
      for (int j = 0; j < k; ++j) o += words[j];
      return o;
    }
  };
  size_t cap;
  std::vector<Round> rounds;
  std::vector<std::array<size_t, K>> at;  // per item: where its part starts inside each region of its round
  size_t buffer_words = 1;                // the largest round (at least 1)
  size_t stage_words[K];                  // per region, the largest over the rounds (at least 1): what a host staging block needs
  int round_items = 1;                    // the most items of a round

  RegionRounds(size_t cap_words, size_t n_items) : cap(cap_words) {
    at.reserve(n_items);
    for (size_t& s : stage_words) s = 1;
  }
  // the next item, by its region lengths
  void add(const size_t (&w)[K]) {
    size_t item_words = 0;
    for (size_t v : w) item_words += v;
    if (rounds.empty() || used + item_words > cap) {
      rounds.push_back(Round{(int)at.size(), (int)at.size(), {}});
      used = 0;
    }
    Round& rd = rounds.back();
    std::array<size_t, K> o;
    for (int k = 0; k < K; ++k) {
      o[k] = rd.words[k];
      rd.words[k] += w[k];
      stage_words[k] = std::max(stage_words[k], rd.words[k]);
    }
    at.push_back(o);
    rd.q1 = (int)at.size();
    used += item_words;
    buffer_words = std::max(buffer_words, used);
    round_items = std::max(round_items, rd.q1 - rd.q0);
  }

 private:
  size_t used = 0;
};

// Rows of items q0 .. q1-1 through a chunk buffer of `cap` doubles, in pieces of whole quanta of rows (the last piece of an item
// takes what is left).  item_of(q) says what the item brings; piece(q, row0, rows, offset) is called for every piece, `offset` its
// place in the chunk in doubles; flush() is called where the pieces so far are one launch — in front of a piece that finds no room for
// a quantum or finds `max_pieces` pieces waiting, and behind the last piece.  cap >= quantum · per_row of every item: a piece always fits.
struct RowPieces {
  struct Item {
    int rows;        // the item's rows
    size_t per_row;  // doubles a row
    bool takes_part;
  };
  size_t cap;
  int quantum, max_pieces;

  template <class ItemOf, class Piece, class Flush>
  void cut(int q0, int q1, ItemOf item_of, Piece piece, Flush flush) const {
    size_t used = 0;
    int count = 0;
    auto flush_some = [&] {
      if (count == 0) return;
      flush();
      used = 0;
      count = 0;
    };
    for (int q = q0; q < q1; ++q) {
      const Item it = item_of(q);
      if (!it.takes_part) continue;
      const size_t per_q = (size_t)quantum * it.per_row;
      for (int row0 = 0; row0 < it.rows;) {
        if (cap - used < per_q || count == max_pieces) flush_some();
        const size_t fit = (cap - used) / per_q * (size_t)quantum;
        const int rows = (int)std::min<size_t>(fit, (size_t)(it.rows - row0));
        piece(q, row0, rows, used);
        used += (size_t)rows * it.per_row;
        ++count;
        row0 += rows;
      }
    }
    flush_some();
  }
};

}  // namespace icp
