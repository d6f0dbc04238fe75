// scan.h -- Engine::exclusive_sum_total: the count -> exclusive sum -> total step of a selection that leaves the engine as coordinate arrays
// (device_io.hip: the bond graph; pair_graph.hip: the 10 A list).  Only those units include it: engine.h keeps hipcub out of every other one.
// The scans on the step's path (lists.hip, exchange.hip, engine.hip) run in the scratch sized at set-up and have their own host waits.
#pragma once
#include "engine.h"

#include <hipcub/hipcub.hpp>

#include <cstring>

namespace rxmd {

template <class T>
long long Engine::exclusive_sum_total(T *cnt, T *off, int n) {
  static_assert(sizeof(T) <= 8, "the pinned slot holds 8 bytes");
  size_t need = 0;
  RX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, need, cnt, off, n + 1, stream));
  if (need > cubtmp_bytes) {                         // (sized at set-up for NB + 1 items; a dense box has more bonds than atom slots)
    regrow_group(G_CUBTMP, need + 256);
    cubtmp_bytes = need + 256;                       // (only once the larger block exists: the scans of the step's path pass it as the temp size)
  }
  size_t tb = cubtmp_bytes;
  RX_HIP(hipcub::DeviceScan::ExclusiveSum(cubtmp, tb, cnt, off, n + 1, stream));
  RX_HIP(hipMemcpyAsync(h_cnt + H_CNT_EXPORT, off + n, sizeof(T), hipMemcpyDeviceToHost, stream));
  sync_stream();
  T total;
  std::memcpy(&total, h_cnt + H_CNT_EXPORT, sizeof(T));
  return total;
}

}  // namespace rxmd
