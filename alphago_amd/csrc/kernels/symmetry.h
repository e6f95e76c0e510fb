// The D4 board symmetries as the kernels index them (pack.hip: training augmentation; symmetry.hip:
// inference ensembling).
#pragma once
#include <hip/hip_runtime.h>

namespace agk {

// Symmetry s maps board point (x, y) to (x', y'); numpy semantics of the
// reference BOARD_TRANSFORMATIONS on a [x][y] array.
__device__ __forceinline__ void sym_fwd(int s, int n, int x, int y, int& ox, int& oy) {
  switch (s) {
    case 1: ox = n - 1 - y; oy = x; break;          // rot90
    case 2: ox = n - 1 - x; oy = n - 1 - y; break;  // rot180
    case 3: ox = y; oy = n - 1 - x; break;          // rot270
    case 4: ox = x; oy = n - 1 - y; break;          // fliplr
    case 5: ox = n - 1 - x; oy = y; break;          // flipud
    case 6: ox = y; oy = x; break;                  // transpose
    case 7: ox = n - 1 - y; oy = n - 1 - x; break;  // fliplr(rot90)
    default: ox = x; oy = y; break;
  }
}
__device__ __forceinline__ void sym_inv(int s, int n, int i, int j, int& x, int& y) {
  switch (s) {
    case 1: x = j; y = n - 1 - i; break;
    case 3: x = n - 1 - j; y = i; break;
    default: sym_fwd(s, n, i, j, x, y); break;  // the others are involutions
  }
}

}  // namespace agk
