// nwk_sched.h -- the pure parts of the batch scheduler of nwk_runtime.cpp:
// which pairs go into one batch (form_batch) and in which order a batch's band
// tasks are dequeued (order_tasks).  Host only, no device call and no nwk_ctx,
// so tests/native/host_selftest.cpp checks them without a GPU: a band that is
// missing, duplicated or out of order hangs a persistent kernel.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "nwk_internal.h"

namespace nwk {

// HBM footprint of one pair, or (summed) of a batch.
struct Footprint {
  int64_t mat_dw, bnd_gr, ops_b;  // matrix dwords, boundary granules, op-string bytes
  int64_t segops_b, segctl_b;     // segmented traceback: move buffers, control (flags, info, records)
  // bytes of d_work and d_segctl: the op strings count three times (moves and
  // the device finalize's two rows), 8192 covers the regions' alignment slack
  int64_t need() const { return mat_dw * 4 + bnd_gr * 8 + 3 * ops_b + segops_b + segctl_b + 8192; }
  // ... of a batch of footprint *this with pair w added
  int64_t need_with(const Footprint& w) const {
    Footprint s = *this;
    s += w;
    return s.need();
  }
  Footprint& operator+=(const Footprint& w) {
    mat_dw += w.mat_dw; bnd_gr += w.bnd_gr; ops_b += w.ops_b; segops_b += w.segops_b; segctl_b += w.segctl_b;
    return *this;
  }
};

// The batch that starts at pair `pos`: pairs [pos, end) with footprint `sum`.
// linear: pair `pos` does not fit the budget even alone (or lin_all: every
// pair takes the linear-space path); then end == pos, nothing is consumed, and
// need is what pair `pos` asked for.
struct BatchCut {
  size_t end;
  Footprint sum;
  bool linear;
  int64_t need;
};

// W: a type derived from Footprint (PairWork).  Takes pairs in order while the
// batch's need() does not exceed the budget.
template <class W>
BatchCut form_batch(const W* w, size_t pos, size_t n, int64_t budget, bool lin_all) {
  BatchCut b{pos, Footprint{}, false, 0};
  while (b.end < n) {
    const int64_t need = b.sum.need_with(w[b.end]);
    if (need > budget || lin_all) {
      if (b.end == pos) b.linear = true, b.need = need;
      break;
    }
    b.sum += w[b.end];
    ++b.end;
  }
  return b;
}

// The task list of a batch of np pairs: {pair, band} entries in dequeue order.
// ntk[q]: tasks of pair q -- its bands (or band pairs, kPacked2 / kAffinePk:
// task b is the b-th band pair), or with `paired` (kCol paired tasks)
// (nbands[q] + 1) / 2: task b fills bands 2b and 2b + 1 and carries
// kColTaskPair, an odd last band stays a single.
// order 0: pair-major; 1: band-major; g >= 2: groups of g pairs, band-major
// inside a group.  A pair's tasks always appear in ascending order (a band
// waits on the one above it).  Returns the number of entries, sum of ntk.
inline int64_t order_tasks(const int* nbands, const int* ntk, int np, int order, bool paired, int2* out) {
  int64_t t = 0;
  auto entry = [&](int q, int b) {
    if (!paired) return make_int2(q, b);
    return make_int2(q, 2 * b + 1 < nbands[q] ? (2 * b) | kColTaskPair : 2 * b);
  };
  const int group = order == 0 ? 1 : order == 1 ? std::max(np, 1) : order;
  for (int g0 = 0; g0 < np; g0 += group) {
    const int g1 = std::min(np, g0 + group);
    int mb = 0;
    for (int q = g0; q < g1; ++q) mb = std::max(mb, ntk[q]);
    for (int b = 0; b < mb; ++b)
      for (int q = g0; q < g1; ++q)
        if (b < ntk[q]) out[t++] = entry(q, b);
  }
  return t;
}

}  // namespace nwk
