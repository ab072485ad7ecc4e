// The walk back of csrc/dtw.hip from the corner (Ta-1, Tb-1) along the direction bytes (0 diagonal, 1 up, 2 left; cell (i, j) at
// ((i + j) % Tb) * Ta + i), apart from the kernel so that a host program can hand it bytes that no launch would write
// (tests/test_dtw_cpu.py).  n is the carried length L(Ta-1, Tb-1): path[n - 1] .. path[0] receive (i, j), the corner first.  Whatever
// the bytes and n hold, the walk leaves row 0 and column 0 one way only, so i and j stay inside the pair; it writes at most
// Ta + Tb - 1 entries and stops at (0, 0).  Returns the index of the last entry written (0 when n is the walked length).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SATT_DTW_HD __host__ __device__
#else
#define SATT_DTW_HD
#endif

SATT_DTW_HD inline int dtw_walk_back(const uint8_t* dirs, int Ta, int Tb, int n, int32_t* path) {
  const int nd = Ta + Tb - 1;
  int i = Ta - 1, j = Tb - 1, s = (n < nd ? n : nd) - 1;
  for (; s >= 0; --s) {
    path[2 * s] = i;
    path[2 * s + 1] = j;
    if (i == 0 && j == 0) break;
    const int dir = dirs[(size_t)((i + j) % Tb) * Ta + i];
    if (i == 0) --j;                                              // row 0 and column 0 leave one way, whatever the byte says
    else if (j == 0) --i;
    else if (dir == 0) { --i; --j; }
    else if (dir == 1) --i;
    else --j;
  }
  return s < 0 ? 0 : s;
}
