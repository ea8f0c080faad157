// hipcub's temporary storage for a workspace that sorts n (Key, int32) pairs on `bits` key bits and scans n int32: the larger
// of the two queries plus a spare row, one 256-byte block of the layout (graph.hip, filter.hip)
#pragma once
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include "workspace.h"

template <class Key> static size_t ws_cub_bytes(int n, int bits) {
  size_t a = 0, b = 0;
  Key *k = nullptr;
  int32_t *v = nullptr;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, k, v, v, n, 0, bits, (hipStream_t)0);
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, v, v, n, (hipStream_t)0);
  return round_up((a > b ? a : b) + 256, 256);
}
